"""Stage checks of the multilevel preconditioner's set-up (test_pgo_hierarchy_gpu.py on the device's arrays; test_np_reference_system.py on
the reference's own, with planted faults).  A hierarchy is a dict as capi.DiagPgo.hierarchy() returns it.  Every check takes the INPUTS
of one stage from that dict, applies the float64 reference (np_reference.ml_*) to them and compares the stage's OUTPUT in the dict, entry
by entry, with C_H eps x the magnitude the stage's absolute-value twin returns.  It returns a list of Finding(stage, level, ratio, where):
ratio = worst |difference| / bound (inf where the bound is 0 and the difference is not), where = index of that entry.

`fault` plants a defect in the reference side of one stage (np_reference's fault arguments), never in the hierarchy under test."""
import collections

import numpy as np

import np_reference as NP

EPS = np.finfo(np.float64).eps
C_H = 1e3

Finding = collections.namedtuple("Finding", "stage level ratio where")

# The dense kernels compute the tiles on and above the diagonal of a symmetric result and mirror them (pgo_ml_kernels.hip): ml_mult_qyqt
# in 64 x 64 tiles, the Newton-Schulz GEMMs (both) in 32 x 32.  Their inputs are symmetric only to the round-off of the sibling inverses
# (a Gauss-Jordan inverse is symmetric to eps kappa(W), far above C_H eps of a later product), so WHICH half counts is part of what the
# kernels compute, and the reference mirrors the same tiles.  For the same reason the Newton-Schulz GEMMs' left factor is X^T: they read
# X[k][row] "through X's symmetry" (np_reference.ml_newton_schulz, tile given).
CYCLE_TILE = 64
NS_TILE = 32


def mirrored_exactly(X, tile):
    """Every tile below the diagonal is, bit for bit, the transpose of its partner above."""
    b = np.arange(X.shape[0]) // tile
    return bool(np.all((X == X.T) | (b[:, None] == b[None, :])))


def worst(diff, bound):
    """(largest diff / bound, its index); an entry with bound 0 must have diff 0."""
    diff = np.abs(np.asarray(diff, np.float64)); bound = np.broadcast_to(np.asarray(bound, np.float64), diff.shape)
    if diff.size == 0:
        return 0.0, ()
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(diff > 0, diff / bound, 0.0)
    q = np.where(np.isnan(q), np.inf, q)
    k = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[k]), tuple(int(v) for v in k)


def fans_of(h):
    return [lv["fan"] for lv in h["lv"]]


def check_structure(h):
    """ml_plan (host), exact: n_l = ceil(n_{l-1} / fan_l); fans 8, and 4 at level 2 iff agg = 4; the slots of level l+1 are exactly the
    pairs of aggregates joined by a level-l slot, sorted by column."""
    L = h["levels"]
    lv = h["lv"]
    assert len(lv) == L + 1 and lv[0]["n"] == h["rows"]
    for l in range(1, L + 1):
        want = 4 if (l == 2 and h["agg"] == 4) else 8
        assert lv[l]["fan"] == want, "level %d: fan %d, expected %d (agg %d)" % (l, lv[l]["fan"], want, h["agg"])
        assert lv[l]["n"] == -(-lv[l - 1]["n"] // lv[l]["fan"]), "level %d: %d entities over %d children" % (l, lv[l]["n"], lv[l - 1]["n"])
        rp, cc, _ = NP.ml_coarse_structure(lv[l - 1]["row_ptr"], lv[l - 1]["col"], lv[l]["fan"], lv[l]["n"])
        assert np.array_equal(rp, lv[l]["row_ptr"]), "level %d: row_ptr is not that of the aggregates joined by a level-%d slot" % (l, l - 1)
        assert np.array_equal(cc, lv[l]["col"]), "level %d: the slots' columns differ (or are not sorted)" % l
        assert lv[l]["nslots"] == len(cc)


def check_geometry(h, t, R, fault=None):
    """ml_geometry: cen (weights exact) and geo of every level from the poses of the system's rows (t [rows,3] with NaN for an EMPTY row,
    R [rows,3,3]).  Bound per entry C_H eps (|t|_max + |c|); R^T entries C_H eps (products of unit-quaternion components); EMPTY rows zero."""
    fans = fans_of(h)
    cen, geo = NP.ml_geometry(t, R, fans, fault=fault)
    live = ~np.isnan(t).any(1)
    tmax = float(np.abs(t[live]).max()) if live.any() else 0.0
    out = []
    L = h["levels"]
    for l in range(1, L + 1):
        d = h["lv"][l]["cen"]
        assert np.array_equal(d[:, 3], cen[l][:, 3]), "level %d: centroid weights differ at %s" % (l, np.nonzero(d[:, 3] != cen[l][:, 3])[0][:4])
        out.append(Finding("geometry cen", l, *worst(d[:, :3] - cen[l][:, :3], C_H * EPS * (tmax + np.abs(cen[l][:, :3])))))
    g0 = h["lv"][0]["geo"]
    assert np.all(g0[~live] == 0), "an EMPTY row has a nonzero prolongation block"
    par = np.arange(len(t)) // fans[1]
    out.append(Finding("geometry R^T", 0, *worst(g0[:, :9] - geo[0][:, :9], C_H * EPS)))
    out.append(Finding("geometry d", 0, *worst(g0[:, 9:] - geo[0][:, 9:], C_H * EPS * (tmax + np.abs(cen[1][par, :3])) * live[:, None])))
    for l in range(1, L):
        par = np.arange(h["lv"][l]["n"]) // fans[l + 1]
        out.append(Finding("geometry d", l, *worst(h["lv"][l]["geo"] - geo[l], C_H * EPS * (tmax + np.abs(cen[l + 1][par, :3])))))
    return out


def check_galerkin(h, fault=None, levels=None):
    """ml_galerkin: blk, G, M of level l+1 from the dumped level l (blk, G, M, geo).  Bound C_H eps |P|^T |A_l| |P|; the structure is
    check_structure's, so a block without a contribution does not exist.  fault = (l, ("drop", q))."""
    out = []
    for l in range(h["levels"]) if levels is None else levels:
        F, Cc = h["lv"][l], h["lv"][l + 1]
        P = NP.ml_prolong_blocks(l, F["geo"])
        Pa = NP.ml_prolong_blocks(l, F["geo"], absolute=True)
        M = None if l == 0 else F["M"]
        f = fault[1] if (fault is not None and fault[0] == l) else None
        rp, cc, blk, G, Mc = NP.ml_galerkin(F["row_ptr"], F["col"], F["blk"], F["G"], M, P, Cc["fan"], fault=f)
        _, _, blk_a, G_a, M_a = NP.ml_galerkin(F["row_ptr"], F["col"], F["blk"], F["G"], M, Pa, Cc["fan"], absolute=True)
        assert np.array_equal(rp, Cc["row_ptr"]) and np.array_equal(cc, Cc["col"]), "level %d: slot structure" % (l + 1)
        out.append(Finding("galerkin blk", l + 1, *worst(Cc["blk"] - blk, C_H * EPS * blk_a)))
        out.append(Finding("galerkin G", l + 1, *worst(Cc["G"] - G, C_H * EPS * G_a)))
        out.append(Finding("galerkin M", l + 1, *worst(Cc["M"] - Mc, C_H * EPS * M_a)))
    return out


def inverse_bound(W, inv):
    """Entrywise bound of a normwise backward-stable inverse X = (W + dW)^-1, |dW|_2 <= C_H eps |W|_2: to first order X - W^-1 =
    -W^-1 dW W^-1, so |X - W^-1|_ij <= C_H eps |W|_2 |row i of W^-1|_2 |column j of W^-1|_2.  (kappa(W) |W^-1|_ij - the same product with
    the row and column norms replaced by |W^-1|_2 and the entry itself - is no bound where an entry of W^-1 vanishes by cancellation: the
    kernels' Gauss-Jordan exceeded it there by 37x on a 48 x 48 sibling block whose other entries were within 1e-3 of it.)"""
    nW = np.linalg.norm(W, 2, axis=(-2, -1))
    return C_H * EPS * nW[..., None, None] * np.linalg.norm(inv, axis=-1)[..., :, None] * np.linalg.norm(inv, axis=-2)[..., None, :]


def check_inverses(h, fault=None):
    """ml_inverses / ml_top: Winv[l] and top_inv from the dumped level arrays and lambda, against inverse_bound (a backward-stable
    inverse); the rows and columns of padded children are those of the identity, bit for bit.  fault = (l, ("drop", q)): see
    np_reference.ml_sibling_blocks."""
    out = []
    L, lam = h["levels"], h["lam"]
    for l in range(L):
        F = h["lv"][l]
        fan = h["lv"][l + 1]["fan"]
        W, padded = NP.ml_sibling_blocks(l, F["row_ptr"], F["col"], F["blk"], F["G"], F["M"], lam, fan, couple=(l > 0 or h["sibling0"] == 1),
                                             fault=fault[1] if (fault is not None and fault[0] == l) else None)
        inv = np.linalg.inv(W)
        out.append(Finding("sibling inverses", l, *worst(F["Winv"] - inv, inverse_bound(W, inv))))
        eye = np.eye(6 * fan)
        for A, j in zip(*np.nonzero(padded)):
            s = slice(6 * j, 6 * j + 6)
            assert np.array_equal(F["Winv"][A][s, :], eye[s, :]) and np.array_equal(F["Winv"][A][:, s], eye[:, s]), \
                "level %d aggregate %d: padded child %d is not an identity row / column" % (l, A, j)
    T = h["lv"][L]
    A = NP.ml_level_matrix(T["row_ptr"], T["col"], T["blk"], T["G"], T["M"], lam)
    inv = np.linalg.inv(A)
    out.append(Finding("top inverse", L, *worst(h["top_inv"] - inv, inverse_bound(A, inv))))
    return out


def _level_operands(h, l, fault=None):
    F = h["lv"][l]
    fan = h["lv"][l + 1]["fan"]
    S = NP.ml_dense_S(F["Winv"], F["n"], fault=fault if (fault is not None and fault[0] == "transpose") else None)
    P = NP.ml_dense_P(F["geo"], fan)
    Yup = h["top_inv"] if l + 1 == h["levels"] else h["lv"][l + 1]["Y"]
    return S, P, Yup


def check_dense(h, h0=None, fault=None):
    """The dense operators from the top down to cl, each from the DUMPED operator of the level above, Winv and geo.
    Additive (ml_dense_level): Y_l = S + P Y_{l+1} P^T, bound C_H eps (|S| + |P| |Y_{l+1}| |P|^T).
    Multiplicative (ml_mult_pair / _qy / _qyqt, ml_ns_ax / ml_ns_gemm*): levels above cl - the cycle X_0 = 2 S - S A S + Q Y Q^T and its
    upper_ns Newton-Schulz steps as one stage, bounds added; level cl - X_0 of the hierarchy h0 (the same set-up with 0 steps) against the
    cycle's bound C_H eps (2 |S| + |S| |A| |S| + |Q| |Y| |Q|^T) and the exact mirror image of its upper tiles, then Y_cl after ns_steps steps FROM THE DEVICE'S OWN
    X_0, bound C_H eps sum over the steps of (2 |X| + |X| |A| |X|).  The reference mirrors the kernels' tiles (CYCLE_TILE, NS_TILE).  fault (reference side): ("transpose", A, i, j) at level cl's S,
    ("tile", i, j) in Q Y Q^T of level cl, ("skip", k) a Newton-Schulz step of level cl."""
    out = []
    L, cl, lam = h["levels"], h["cl"], h["lam"]
    if not cl:
        return out
    for l in range(L - 1, cl - 1, -1):
        F = h["lv"][l]
        S, P, Yup = _level_operands(h, l, fault if l == cl else None)
        if not h["mult"]:
            ref = NP.ml_additive(S, P, Yup)
            out.append(Finding("additive dense", l, *worst(F["Y"] - ref, C_H * EPS * NP.ml_additive(S, P, Yup, absolute=True))))
            continue
        A = NP.ml_level_matrix(F["row_ptr"], F["col"], F["blk"], F["G"], F["M"], lam)
        cyc_mag = NP.ml_mult_cycle(S, A, P, Yup, absolute=True)
        Z0 = NP.ml_mult_cycle(S, A, P, Yup, fault=fault if (l == cl and fault is not None and fault[0] == "tile") else None)
        X0 = NP.tile_mirror(Z0, CYCLE_TILE)
        assert mirrored_exactly(F["Y"], NS_TILE), "level %d: Y is not the mirror image of its upper 32 x 32 tiles" % l
        if l > cl:
            ref, mag = NP.ml_newton_schulz(X0, A, h["upper_ns"], tile=NS_TILE)
            out.append(Finding("cycle + Newton-Schulz (upper)", l, *worst(F["Y"] - ref, C_H * EPS * (cyc_mag + mag))))
            continue
        if h0 is not None:
            X0d = h0["lv"][cl]["Y"]
            out.append(Finding("multiplicative cycle X0", l, *worst(X0d - X0, C_H * EPS * cyc_mag)))
            # symmetry: exact between mirrored tiles.  Inside a diagonal tile X0 is as symmetric as the sibling inverses it is made of
            # (eps kappa(W)) and no more: the entries there are held by the X0 check above, not by a symmetry bound
            assert mirrored_exactly(X0d, CYCLE_TILE), "level %d: X0 is not the mirror image of its upper 64 x 64 tiles" % l
            skip = fault[1] if (fault is not None and fault[0] == "skip") else None
            ref, mag = NP.ml_newton_schulz(X0d, A, h["ns_steps"], skip=skip, tile=NS_TILE)
            out.append(Finding("Newton-Schulz", l, *worst(F["Y"] - ref, C_H * EPS * mag)))
    return out


def check_cmat32(h):
    """ml_cmat32 / the last GEMM's epilogue: Cmat32[:, :6 n_cl] == float32(Y_cl) bit for bit, pad columns zero."""
    cl = h["cl"]
    if not cl:
        assert h["Cmat32"] is None
        return
    n6 = 6 * h["lv"][cl]["n"]
    C = h["Cmat32"]
    assert C.shape == (n6, (n6 + 3) & ~3) and h["c32_stride"] == C.shape[1]
    want = h["lv"][cl]["Y"].astype(np.float32)
    bad = np.nonzero(C[:, :n6].view(np.uint32) != want.view(np.uint32))
    assert len(bad[0]) == 0, "Cmat32 is not float32(Y_cl) at %d entries, first (%d, %d)" % (len(bad[0]), bad[0][0], bad[1][0])
    assert np.all(C[:, n6:] == 0), "pad columns of Cmat32 are not zero"


def apply_reference(h, x, absolute=False, coarse_from=None):
    """M^-1 x (or its absolute-value twin on |x|) from the dumped Winv, geo, Cmat32 and top_inv."""
    fans = fans_of(h)
    cl = h["cl"]
    stop = cl if cl else h["levels"]
    Pb = [NP.ml_prolong_blocks(l, h["lv"][l]["geo"]) for l in range(stop)]
    Wi = [h["lv"][l]["Winv"] for l in range(stop)]
    Y = h["Cmat32"][:, :6 * h["lv"][cl]["n"]].astype(np.float64) if cl else None
    return NP.ml_apply(x, Pb, Wi, fans, h["top_inv"], cl=cl, Ycl=Y, absolute=absolute, coarse_from=coarse_from)


def restrict_to(h, r, level, absolute=False):
    """P^T r down to `level` (the gather level of the PCG kernels) from the dumped geo."""
    fans = fans_of(h)
    v = np.abs(np.asarray(r, np.float64)).reshape(-1, 6) if absolute else np.asarray(r, np.float64).reshape(-1, 6)
    for l in range(level):
        v = NP.ml_restrict(NP.ml_prolong_blocks(l, h["lv"][l]["geo"], absolute=absolute), v, fans[l + 1])
    return v


def check_steady_state(h, st, b, k, C_R=1e3):
    """The fused iteration after k PCG iterations (ml_spmv's restriction of A p, ml_alpha, ml_cg).  ml_cg does not restrict r: for the
    coarse part of z it uses rg_old - alpha Sg of ALL aggregates (the recurrence), and writes, for the next iteration, the exact
    restriction of its OWN rows' new r.
      * the dumped rg (what the next ml_cg would read) = P^T r of the dumped r, C_H eps |P|^T |r|: this pins the workgroups' own exact
        restriction - the buffer the recurrence starts from - not the recurrence itself;
      * z = M^-1 r carries the recurrence: the application bound, plus - for the part of z that went through the gathered residual
        (the levels from the gather level up) - that part of the absolute-value application applied to the recurrence drift
        C_R eps (k + 1) (|A| |x| + |b|) of check_recurrence_residual (test_pgo_system_gpu.py).  A wrong Sg or alpha is an error of the
        size of r itself: ~1e12 bounds;
      * r itself against b - A x, within that drift (per entry)."""
    lv0 = h["lv"][0]
    n = lv0["n"]
    A = NP.bcsr_to_sparse(lv0["row_ptr"], lv0["col"], lv0["blk"], diag=lv0["G"] + h["lam"] * np.eye(6), nrows=n)
    x, r, z = st["x"].reshape(-1), st["r"], st["z"]
    drift = (C_R * EPS * (k + 1) * (abs(A) @ np.abs(x) + np.abs(b.reshape(-1)))).reshape(-1, 6)
    out = [Finding("steady state: r against b - A x", 0, *worst(r - (b.reshape(-1) - A @ x).reshape(-1, 6), drift))]
    gl = st["gather_level"]
    out.append(Finding("steady state: gather-level residual", gl, *worst(st["rg"] - restrict_to(h, r, gl), C_H * EPS * restrict_to(h, r, gl, absolute=True))))
    bound = C_H * EPS * apply_reference(h, np.abs(r), absolute=True) + apply_reference(h, drift, absolute=True, coarse_from=gl)
    out.append(Finding("steady state: z", 0, *worst(z - apply_reference(h, r), bound)))
    return out


def check_direction(prev2, prev, cur):
    """The direction of iteration j from the states after j - 2, j - 1 and j iterations (prev2 = None: j = 1, p = z_0):
    p_j = z_{j-1} + beta p_{j-1}, beta = r_{j-1}.z_{j-1} / r_{j-2}.z_{j-2} (ml_spmv, from ml_cg's partials).  Bound C_H eps (|z| + B |p|),
    B = the magnitude of beta's terms: (sum |r z|_{j-1} + beta sum |r z|_{j-2}) / r_{j-2}.z_{j-2}."""
    z = prev["z"]
    if prev2 is None:
        return Finding("steady state: direction p", 0, *worst(cur["p"] - z, C_H * EPS * np.abs(z)))
    rz1, rz0 = float((prev["r"] * prev["z"]).sum()), float((prev2["r"] * prev2["z"]).sum())
    beta = rz1 / rz0
    B = (float(np.abs(prev["r"] * prev["z"]).sum()) + abs(beta) * float(np.abs(prev2["r"] * prev2["z"]).sum())) / abs(rz0)
    return Finding("steady state: direction p", 0, *worst(cur["p"] - (z + beta * prev["p"]), C_H * EPS * (np.abs(z) + B * np.abs(prev["p"]))))


def check_apply(h, x, z):
    """One application z = M^-1 x of the PCG's kernels against the reference application of the dumped arrays; bound C_H eps x the
    absolute-value application of |x|."""
    ref = apply_reference(h, x)
    mag = apply_reference(h, x, absolute=True)
    return Finding("application", 0, *worst(np.asarray(z).reshape(-1, 6) - ref, C_H * EPS * mag))


def reference_pcg(A, b, apply, tol, maxit=2000):
    """Float64 PCG with the plain relative stop test of cfg.pcg_stop = 1: the number of iterations after which
    r.M^-1 r <= tol^2 r_0.M^-1 r_0 first holds."""
    b = np.asarray(b, np.float64).reshape(-1)
    x = np.zeros_like(b); r = b.copy()
    z = apply(r.reshape(-1, 6)).reshape(-1)
    p = z.copy(); rz = float(r @ z); thr = tol * tol * rz
    for it in range(1, maxit + 1):
        Ap = A @ p
        a = rz / float(p @ Ap)
        x += a * p; r -= a * Ap
        z = apply(r.reshape(-1, 6)).reshape(-1)
        rzn = float(r @ z)
        if not rzn > thr:
            return it, x
        p = z + (rzn / rz) * p; rz = rzn
    return maxit, x


def reference_hierarchy(row_ptr, col, blk, hdiag, t, R, lam, agg=1, cl=1, mult=1, ns_steps=2, upper_ns=4, sibling0=1, top_max=16, fans=None):
    """A hierarchy dict (the hook's format) made by the float64 reference alone: what a correct device would return, to round-off.
    fans: the fan-outs per level (fans[0] = 1); None: 8 (4 at level 2 when agg = 4) until at most top_max aggregates remain."""
    n = len(row_ptr) - 1
    ns = [n]
    if fans is None:
        fans = [1]
        while ns[-1] > top_max:
            fans.append(4 if (len(fans) == 2 and agg == 4) else 8)
            ns.append(-(-ns[-1] // fans[-1]))
    else:
        fans = list(fans)
        ns = NP.ml_level_sizes(n, fans)
    L = len(fans) - 1
    cen, geo = NP.ml_geometry(t, R, fans)
    live = ~np.isnan(np.asarray(t)).any(1)
    lv = [dict(n=n, fan=1, nslots=len(col), row_ptr=np.asarray(row_ptr), col=np.asarray(col), blk=np.asarray(blk, np.float64).reshape(-1, 6, 6),
               G=np.asarray(hdiag, np.float64).reshape(-1, 6, 6), M=None, geo=geo[0], cen=None, Y=None)]
    for l in range(L):
        F = lv[l]
        P = NP.ml_prolong_blocks(l, F["geo"])
        rp, cc, b, G, M = NP.ml_galerkin(F["row_ptr"], F["col"], F["blk"], F["G"], F["M"], P, fans[l + 1])
        lv.append(dict(n=ns[l + 1], fan=fans[l + 1], nslots=len(cc), row_ptr=rp, col=cc, blk=b, G=G, M=M, geo=geo[l + 1], cen=cen[l + 1], Y=None))
    h = dict(levels=L, cl=cl, agg=agg, mult=mult, ns_steps=ns_steps if mult else 0, upper_ns=upper_ns, sibling0=sibling0, rows=n, lam=lam, lv=lv,
             b2v=np.where(live, np.arange(n), -1), reduced=0, strong=0, strong_blocks=0)
    for l in range(L):
        F = lv[l]
        W, _ = NP.ml_sibling_blocks(l, F["row_ptr"], F["col"], F["blk"], F["G"], F["M"], lam, fans[l + 1], couple=(l > 0 or sibling0 == 1))
        F["Winv"] = np.linalg.inv(W)
    T = lv[L]
    T["Winv"] = None
    h["top_inv"] = np.linalg.inv(NP.ml_level_matrix(T["row_ptr"], T["col"], T["blk"], T["G"], T["M"], lam))
    h0 = None
    if cl:
        for l in range(L - 1, cl - 1, -1):
            F = lv[l]
            S, P, Yup = _level_operands(h, l)
            if not mult:
                F["Y"] = NP.ml_additive(S, P, Yup)
                continue
            A = NP.ml_level_matrix(F["row_ptr"], F["col"], F["blk"], F["G"], F["M"], lam)
            X0 = NP.ml_mult_cycle(S, A, P, Yup, tile=CYCLE_TILE)
            if l == cl:
                h0 = dict(h, lv=[dict(x) for x in lv]); h0["lv"][cl]["Y"] = X0; h0["ns_steps"] = 0
            F["Y"], _ = NP.ml_newton_schulz(X0, A, upper_ns if l > cl else ns_steps, tile=NS_TILE)
        n6 = 6 * lv[cl]["n"]
        C = np.zeros((n6, (n6 + 3) & ~3), np.float32)
        C[:, :n6] = lv[cl]["Y"].astype(np.float32)
        h["Cmat32"] = C; h["c32_stride"] = C.shape[1]
        if h0 is not None:
            C0 = np.zeros_like(C); C0[:, :n6] = h0["lv"][cl]["Y"].astype(np.float32); h0["Cmat32"] = C0; h0["c32_stride"] = C.shape[1]
    else:
        h["Cmat32"] = None; h["c32_stride"] = 0
    return h, h0
