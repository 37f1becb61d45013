"""NumPy restatement of uzl_pgo_rewrite_graph's contract (include/uzl_mi355x.h): the index part of uzliti_slam_amd.merge.apply_merge_plan
generalised to a list of dropped nodes and to ops on either side of an edge, and the same over the solver's uzl_edge arrays.  Written
from the contract, not from csrc/pgo_structure.hip: tests/test_pgo_rewrite_plan_cpu.py and tests/test_pgo_rewrite_gpu.py compare against it."""
import numpy as np

from uzliti_slam_amd import capi
from uzliti_slam_amd.merge import _compose

KEEP_FROM, KEEP_TO, RETARGET_FROM, RETARGET_TO, DELETE = (capi.MERGE_EDGE_KEEP_FROM, capi.MERGE_EDGE_KEEP_TO, capi.MERGE_EDGE_RETARGET_FROM,
                                                          capi.MERGE_EDGE_RETARGET_TO, capi.MERGE_EDGE_DELETE)


def op_rows(ops):
    """ops as rows (edge, action, xf, node), from rows or a capi.PGO_EDGE_OP_DTYPE array"""
    if isinstance(ops, np.ndarray) and ops.dtype == capi.PGO_EDGE_OP_DTYPE:
        return np.stack([ops["edge"], ops["action"], ops["xf"], ops["node"]], axis=1).astype(np.int64).reshape(-1, 4)
    return np.asarray(ops, np.int64).reshape(-1, 4)


def restate_index(n, frm, to, drop_nodes=(), ops=()):
    """-> dict(old_to_new_node, new_to_old_node, old_to_new_edge, new_to_old_edge, rec [e_new, 4] = (from_new, to_new, xf_from, xf_to))"""
    frm, to = np.array(frm, np.int64).reshape(-1), np.array(to, np.int64).reshape(-1)
    ne = len(frm)
    dropped = np.zeros(n, bool)
    dropped[np.asarray(drop_nodes, np.int64).reshape(-1)] = True
    old_to_new_node = np.where(dropped, -1, np.cumsum(~dropped) - 1).astype(np.int32)
    xf_from, xf_to, deleted = -np.ones(ne, np.int64), -np.ones(ne, np.int64), np.zeros(ne, bool)
    for e, a, x, node in op_rows(ops):
        if a == DELETE:
            deleted[e] = True
        elif a in (KEEP_FROM, RETARGET_FROM):
            xf_from[e] = x
            if a == RETARGET_FROM:
                frm[e] = node
        elif a in (KEEP_TO, RETARGET_TO):
            xf_to[e] = x
            if a == RETARGET_TO:
                to[e] = node

    def inside(v):
        return (v >= 0) & (v < n)

    def names_dropped(v):
        return inside(v) & dropped[np.clip(v, 0, max(n - 1, 0))] if n else np.zeros(len(v), bool)

    def renumber(v):
        return np.where(inside(v), old_to_new_node[np.clip(v, 0, max(n - 1, 0))], v) if n else v

    alive = ~deleted & ~names_dropped(frm) & ~names_dropped(to)
    old_to_new_edge = np.where(alive, np.cumsum(alive) - 1, -1).astype(np.int32)
    rec = np.stack([renumber(frm)[alive], renumber(to)[alive], xf_from[alive], xf_to[alive]], axis=1).astype(np.int32).reshape(-1, 4)
    return dict(old_to_new_node=old_to_new_node, new_to_old_node=np.flatnonzero(~dropped).astype(np.int32), old_to_new_edge=old_to_new_edge,
                new_to_old_edge=np.flatnonzero(alive).astype(np.int32), rec=rec)


def rewrite_arrays(poses, fixed, edges, drop_nodes=(), pose_nodes=(), new_poses=None, xf=None, ops=()):
    """The rewrite over the arrays capi.Pgo.add_graph takes (edges: dict of arrays as synth.make_pose_graph makes it)
    -> (poses (n_new, 12), fixed, edges dict, old_to_new_node, old_to_new_edge): what a fresh handle is given for the rewritten graph"""
    P = np.array(poses, np.float64).reshape(-1, 12)
    n = len(P)
    ix = restate_index(n, edges["from"], edges["to"], drop_nodes, ops)
    if len(pose_nodes):
        P[np.asarray(pose_nodes, np.int64)] = np.asarray(new_poses, np.float64).reshape(-1, 12)
    X = np.asarray(xf if xf is not None else [], np.float64).reshape(-1, 12)
    keep_e = ix["new_to_old_edge"]
    out = {k: np.array(np.asarray(v)[keep_e]) for k, v in edges.items()}
    out["displacement_from"] = np.array(out["displacement_from"], np.float64).reshape(-1, 12)
    out["displacement_to"] = np.array(out["displacement_to"], np.float64).reshape(-1, 12)
    for k, (f, t, xf_from, xf_to) in enumerate(ix["rec"]):
        out["from"][k] = f; out["to"][k] = t
        if xf_from >= 0:
            out["displacement_from"][k] = _compose(X[xf_from], out["displacement_from"][k])
        if xf_to >= 0:
            out["displacement_to"][k] = _compose(X[xf_to], out["displacement_to"][k])
    keep_n = ix["new_to_old_node"]
    return P[keep_n], np.asarray(fixed)[keep_n], out, ix["old_to_new_node"], ix["old_to_new_edge"]
