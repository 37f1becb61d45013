"""The rules of a pose graph's structure (csrc/pgo_structure.hpp) restated in NumPy from their comments, for test_pgo_structure_plan.py and
test_pgo_structure_gpu.py: not the code under test.  Flatten and gauge have the oracle as their reference (oracle.flatten_graph,
oracle.set_fixed_nodes); the graph shapes both test modules use are here too."""
import numpy as np

import ml_classes as MC

ROW_HDR = 24                    # kRowHdr
STRONG_MIN = 32                 # kSchurStrongMin
SCHUR_MIN_PCT = 33              # kSchurMinPct


def in_edges_of(g):
    """(from, to, odom, valid) and the trace of the information matrix of every input edge of a synth graph: what uzl_pgo_add_graph keeps."""
    from uzliti_slam_amd import synth
    e = g["edges"]
    ie = np.stack([np.asarray(e["from"]), np.asarray(e["to"]), np.asarray(e["type"]) == synth.EDGE_TYPE_ODOM, np.asarray(e["valid"]) != 0], 1)
    info = np.asarray(e["information"], np.float64).reshape(-1, 6, 6)
    return ie.astype(np.int32), np.trace(info, axis1=1, axis2=2)


def aggregation_order(n, ij, fixed, w=None):
    """From the lowest-index unvisited free vertex follow the heaviest edge to an unvisited free vertex until stuck (ties: the lower
    index), then extend the same chain backwards from the start; repeat."""
    ij = np.asarray(ij).reshape(-1, 2)
    w = np.ones(len(ij)) if w is None else np.asarray(w, np.float64)
    nbrs = [[] for _ in range(n)]
    for (a, b), x in zip(ij.tolist(), w.tolist()):
        if not fixed[a] and not fixed[b]:
            nbrs[a].append((x, b)); nbrs[b].append((x, a))
    seen = np.zeros(n, bool)

    def walk(v):
        out = []
        while True:
            cand = [(-x, u) for x, u in nbrs[v] if not seen[u]]
            if not cand:
                return out
            v = min(cand)[1]
            seen[v] = True; out.append(v)

    order = []
    for start in range(n):
        if fixed[start] or seen[start]:
            continue
        seen[start] = True
        fwd = walk(start)
        back = walk(start)
        order += back[::-1] + [start] + fwd
    return np.asarray(order, np.int32)


def block_csr(n, ij, robust, b2v):
    """test_ml_plan.csr for a given order of the free vertices, with what hangs on a slot: one slot per (free endpoint, edge), in edge
    order within a row; col = -1 for a fixed neighbour; slot_edge = 2 k for edge k in its first endpoint's row, 2 k + 1 in its second's;
    smeta = (slot_edge, i, j, (the edge's slot in the other row + 1, 0 if that endpoint is fixed) | robust << 30)."""
    ij = np.asarray(ij, np.int64).reshape(-1, 2); b2v = np.asarray(b2v, np.int64)
    nb = len(b2v)
    v2b = np.full(max(n, 0), -1, np.int64); v2b[b2v] = np.arange(nb)
    row = v2b[ij].reshape(-1)
    col = v2b[ij[:, ::-1]].reshape(-1)
    keep = np.nonzero(row >= 0)[0]
    order = keep[np.argsort(row[keep], kind="stable")]          # slot -> 2 k + side
    rp = np.zeros(nb + 1, np.int64); np.cumsum(np.bincount(row[keep], minlength=nb), out=rp[1:])
    slot_of = np.full(2 * len(ij), -1, np.int64); slot_of[order] = np.arange(len(order))
    k = order >> 1
    partner = slot_of[order ^ 1] + 1
    smeta = np.stack([order, ij[k, 0], ij[k, 1], partner | (np.asarray(robust, np.int64)[k] != 0) << 30], 1) if len(order) else np.zeros((0, 4), np.int64)
    i32 = lambda a: a.astype(np.int32)
    return dict(nb=nb, nslots=len(order), v2b=i32(v2b), row_ptr=i32(rp), col=i32(col[order]), slot_edge=i32(order), smeta=i32(smeta))


def row_caps(nb, nslots, max_partials=MC.MAX_PARTIALS):
    """<= 256 slots and <= 42 rows per block; beyond max_partials blocks, more: half the partials each for the slot and for the row cap,
    the slot cap in steps of 256"""
    half = max_partials // 2
    cap_slots = max(256, -(-(-(-nslots // half)) // 256) * 256)
    return cap_slots, max(42, -(-nb // half))


def row_blocks(row_ptr, max_partials=MC.MAX_PARTIALS):
    """consecutive rows while the block stays within both caps; a row above the slot cap is a block of its own"""
    rp = np.asarray(row_ptr, np.int64); nb = len(rp) - 1
    cap_slots, cap_rows = row_caps(nb, int(rp[nb]), max_partials)
    out, first = [0], 0
    for a in range(nb):
        if a > first and (a - first >= cap_rows or rp[a + 1] - rp[first] > cap_slots):
            out.append(a); first = a
    out.append(nb)
    return np.asarray(out, np.int32)


def row_headers(row_ptr, col):
    """[max(nb, 1)][24] = (row_ptr[a], row_ptr[a + 1], col of the first 20 slots, -1 past the end and in the pad)"""
    rp = np.asarray(row_ptr, np.int64); nb = len(rp) - 1
    hdr = np.full((max(nb, 1), ROW_HDR), -1, np.int32)
    for a in range(nb):
        c = np.asarray(col[rp[a]:min(rp[a + 1], rp[a] + 20)])
        hdr[a, 0], hdr[a, 1] = rp[a], rp[a + 1]; hdr[a, 2:2 + len(c)] = c
    return hdr


def reduced_numbering(cfg_numbering, preconditioner, may_shard, num_its):
    """-> (strong_min, max_contig): 1 = row order, 2 = strong aggregates, 0 = the handle chooses - by what its own solves measured (the
    cheaper of the two figures; one figure: above 40 iterations per trial try the other), the first structure by the shape of the groups
    (max_contig 0.6).  A sharded solve and block-Jacobi take the row order whatever is asked."""
    if may_shard or preconditioner == 0 or cfg_numbering == 1:
        return 0, 2.0
    if cfg_numbering == 2:
        return STRONG_MIN, 2.0
    ir, is_ = num_its
    if ir >= 0 and is_ >= 0:
        return (STRONG_MIN if is_ < ir else 0), 2.0
    if ir >= 0:
        return (STRONG_MIN if ir > 40 else 0), 2.0
    if is_ >= 0:
        return (0 if is_ > 40 else STRONG_MIN), 2.0
    return STRONG_MIN, 0.6


def schur_min_int(nb):
    """the smallest count of eliminated rows that is >= 64 and >= 33 % of nb"""
    return max(64, -(-SCHUR_MIN_PCT * nb // 100))


def schur_admitted(nb, n_int):
    return n_int >= 64 and 100 * n_int >= SCHUR_MIN_PCT * nb


def shard_range(e, rank, world):
    """contiguous ranges, the first e % world ranks one edge more; the diagonal's owner is rank 0"""
    lo = [r * (e // world) + min(r, e % world) for r in range(world + 1)]
    return lo[rank], lo[rank + 1], 1 if rank == 0 else 0


def exchange_layout(nbp, plan):
    """[A p (6 nbp) | restricted A p (6 n_g; gather level 2: two parts per entity) | one p.Ap partial per ml_spmv workgroup]; plan: capi.ml_plan's dict"""
    gl = plan["gather_level"] if plan["levels"] else 0
    ng6 = plan["lv"][gl]["n"] * 6 * (2 if gl == 2 else 1) if gl else 0
    return dict(sg=6 * nbp, part_a=6 * nbp + ng6, iter_span=6 * nbp + ng6 + (MC.spmv_groups(nbp, plan["agg"]) if gl else 0))


def edges_survive_in_order(old_ij, new_ij, window=4096):
    """the plain double loop: nine in ten old edges found in order in the new list, each at most `window` ahead of the last one found"""
    old = np.asarray(old_ij).reshape(-1, 2).tolist(); new = np.asarray(new_ij).reshape(-1, 2).tolist()
    at = found = 0
    for a, c in old:
        for q in range(at, min(len(new), at + window)):
            if new[q] == [a, c]:
                found += 1; at = q + 1
                break
    return 10 * found >= 9 * len(old)


def graph_grown(old, new, window=4096):
    (n0, f0, ij0), (n1, f1, ij1) = old, new
    return n1 >= n0 and np.array_equal(np.asarray(f0)[:n0], np.asarray(f1)[:n0]) and edges_survive_in_order(ij0, ij1, window)


# ------------------------------------------------------------------------------------------------------------------ graph shapes
def skip_rule_graph():
    """12 nodes, nodes 0 and 5 fixed, a chain of odometry edges and one of every kind of edge the skip rules drop (and their kept
    twins): -> synth-shaped graph dict"""
    from uzliti_slam_amd import synth
    g = synth.make_pose_graph(12, 30, seed=5)
    e = {k: np.array(v) for k, v in g["edges"].items()}
    odo, feat = synth.EDGE_TYPE_ODOM, synth.EDGE_TYPE_3D_FULL
    fixed = np.zeros(12, np.uint8); fixed[[0, 5]] = 1
    rows = [(3, 12, feat, 1), (-1, 4, odo, 1),        # out-of-range endpoints
            (4, 4, feat, 1),                          # self edge
            (2, 7, feat, 0),                          # invalid feature edge
            (2, 7, feat, 1),                          # ... and its valid twin
            (5, 6, odo, 1),                           # odometry from a fixed to a free node: dropped
            (6, 5, odo, 1),                           # ... free to fixed: kept
            (0, 5, feat, 1),                          # feature edge between two fixed nodes: dropped
            (0, 5, odo, 1),                           # ... odometry between two fixed nodes: kept
            (5, 9, feat, 1)]                          # feature edge from a fixed node: kept
    k = len(rows)
    assert len(e["from"]) >= k
    sel = np.arange(len(e["from"]) - k, len(e["from"]))
    for q, (a, b, t, v) in zip(sel, rows):
        e["from"][q], e["to"][q], e["type"][q], e["valid"][q] = a, b, t, v
    return dict(g, nodes_fixed=fixed, edges=e)


def hub_graph(arms=300):
    """one free hub with `arms` feature edges to free leaves that also hang on a chain: the hub's row has `arms` slots"""
    n = arms + 2
    chain = np.stack([np.arange(1, n - 1), np.arange(2, n)], 1)
    hub = np.stack([np.full(arms, 1), np.arange(2, n)], 1)
    ij = np.concatenate([[[0, 2]], chain[1:], hub]).astype(np.int32)
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    return n, fixed, ij, np.ones(len(ij), np.uint8)
