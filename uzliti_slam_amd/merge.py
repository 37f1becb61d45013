"""Applying a merge plan (capi.Merge.plan, uzl_merge_plan).  apply_merge_plan rewrites the caller's arrays: the compacted arrays it
returns go to the set_graph of the gate, scope and merge handles (and are the host restatement of the rewrite).  The solver's resident
graph takes a merge or a scope drop in place: pgo_rewrite_of_plan / pgo_rewrite_of_drops make the arguments of capi.Pgo.rewrite_graph."""
import numpy as np

from . import capi


def _compose(A, B):
    """A * B of two 3 x 4 transforms [R|t] (12 doubles, row-major): rows of A times columns of B, summed left to right"""
    out = np.empty(12)
    for i in range(3):
        a0, a1, a2, a3 = float(A[4 * i]), float(A[4 * i + 1]), float(A[4 * i + 2]), float(A[4 * i + 3])
        for j in range(3):
            out[4 * i + j] = (a0 * float(B[j]) + a1 * float(B[4 + j])) + a2 * float(B[8 + j])
        out[4 * i + 3] = ((a0 * float(B[3]) + a1 * float(B[7])) + a2 * float(B[11])) + a3
    return out


def apply_merge_plan(poses, edges, displacements, plan):
    """poses (n,12); edges: GATE_EDGE_DTYPE array; displacements: (displacement_from (e,12), displacement_to (e,12)) or None for
    identities; plan: what Merge.plan(keep, drop, ...) returned for this graph.
    -> (poses (n-1,12), edges, (displacement_from, displacement_to), old_to_new (n) int32) with node `drop` gone, the nodes behind it
    one index lower (old_to_new[drop] = -1), keep at the plan's new pose, every edge action applied and the deleted edges dropped;
    the edges keep their order.  An edge that still names `drop` afterwards (a retargeted self-loop of it) goes with the node."""
    P = np.array(poses, np.float64).reshape(-1, 12)
    E = np.array(np.ascontiguousarray(edges, capi.GATE_EDGE_DTYPE))
    n, ne = len(P), len(E)
    keep, drop, action = int(plan["keep"]), int(plan["drop"]), np.asarray(plan["action"])
    if not (0 <= keep < n and 0 <= drop < n and keep != drop) or len(action) != ne:
        raise ValueError("the plan does not belong to this graph")
    if displacements is None:
        eye = np.eye(3, 4).reshape(12)
        D_from, D_to = np.tile(eye, (ne, 1)), np.tile(eye, (ne, 1))
    else:
        D_from = np.array(displacements[0], np.float64).reshape(ne, 12)
        D_to = np.array(displacements[1], np.float64).reshape(ne, 12)
    old_to_new = np.arange(n, dtype=np.int32)
    old_to_new[drop + 1:] -= 1
    old_to_new[drop] = -1
    P[keep] = plan["new_pose"]
    for k in np.flatnonzero(action != capi.MERGE_EDGE_UNTOUCHED):
        a = action[k]
        if a == capi.MERGE_EDGE_KEEP_FROM:
            D_from[k] = _compose(plan["keep_displacement"], D_from[k])
        elif a == capi.MERGE_EDGE_KEEP_TO:
            D_to[k] = _compose(plan["keep_displacement"], D_to[k])
        elif a == capi.MERGE_EDGE_RETARGET_FROM:
            D_from[k] = _compose(plan["drop_displacement"], D_from[k]); E["from"][k] = keep
        elif a == capi.MERGE_EDGE_RETARGET_TO:
            D_to[k] = _compose(plan["drop_displacement"], D_to[k]); E["to"][k] = keep
    alive = (action != capi.MERGE_EDGE_DELETE) & (E["from"] != drop) & (E["to"] != drop)
    E = E[alive]
    E["from"] = old_to_new[E["from"]]; E["to"] = old_to_new[E["to"]]
    return np.delete(P, drop, axis=0), E, (D_from[alive], D_to[alive]), old_to_new


def pgo_rewrite_of_plan(plan):
    """The merge plan as the arguments of capi.Pgo.rewrite_graph (uzl_pgo_rewrite_graph): the solver's resident graph takes the merge
    in place, p.rewrite_graph(**pgo_rewrite_of_plan(plan)).  drop leaves, keep takes new_pose, xf = [keep_displacement,
    drop_displacement], one op per edge the plan touches.
    Precondition: the edge order of the merge handle the plan came from is the solver's input-edge order (the edges of add_graph, then
    those of every append_graph, less what earlier rewrites removed) - plan["action"][k] is applied to the solver's input edge k."""
    keep, drop, action = int(plan["keep"]), int(plan["drop"]), np.asarray(plan["action"])
    ops = np.zeros(int((action != capi.MERGE_EDGE_UNTOUCHED).sum()), capi.PGO_EDGE_OP_DTYPE)
    touched = np.flatnonzero(action != capi.MERGE_EDGE_UNTOUCHED)
    ops["edge"] = touched; ops["action"] = action[touched]; ops["node"] = keep
    ops["xf"] = np.isin(action[touched], (capi.MERGE_EDGE_RETARGET_FROM, capi.MERGE_EDGE_RETARGET_TO))        # (0 keep_displacement, 1 drop_displacement)
    return dict(drop_nodes=np.array([drop], np.int32), pose_nodes=np.array([keep], np.int32),
                poses=np.asarray(plan["new_pose"], np.float64).reshape(1, 12),
                xf=np.stack([np.asarray(plan["keep_displacement"], np.float64), np.asarray(plan["drop_displacement"], np.float64)]).reshape(2, 12), ops=ops)


def pgo_rewrite_of_drops(nodes):
    """Nodes that leave the local scope (capi.Scope.request) as the arguments of capi.Pgo.rewrite_graph: they go, and with them every
    edge that names one of them (removeNode, graph_slam_node.cpp:636-660); nothing else is touched."""
    return dict(drop_nodes=np.ascontiguousarray(nodes, np.int32).reshape(-1))


SENSOR_TYPE_FEATURE, SENSOR_TYPE_BINARY_GIST, SENSOR_TYPE_LASERSCAN = 1, 3, 4       # graph_slam_msgs/msg/SensorData.msg:3-6
SENSOR_MERGE, SENSOR_MOVE, SENSOR_DISCARD = "merge", "move", "discard"


def sensor_moves(keep_types, drop_types):
    """The sensor-data loop of mergeNodes (graph_slam_node.cpp:993-1045) over the sensor types of the two nodes, in their
    sensor_data_ order.  -> one (action, j) per sensor of drop:
      (SENSOR_MERGE, j)    a laser scan: merged into keep's sensor j, the first laser scan of keep's list as it stands then
                           (capi.ScanMerge; its displacement becomes drop_displacement * displacement first)
      (SENSOR_MOVE, j)     appended to keep as its sensor j with displacement = drop_displacement * displacement
      (SENSOR_DISCARD, -1) keep already has features / a gist descriptor, or the type is none of the three
    keep's list grows while the loop runs: a second laser scan of drop merges into the one just moved."""
    have = [int(t) for t in keep_types]
    out = []
    for t in (int(t) for t in drop_types):
        if t not in (SENSOR_TYPE_LASERSCAN, SENSOR_TYPE_FEATURE, SENSOR_TYPE_BINARY_GIST):
            out.append((SENSOR_DISCARD, -1))
        elif t in have:
            out.append((SENSOR_MERGE, have.index(t)) if t == SENSOR_TYPE_LASERSCAN else (SENSOR_DISCARD, -1))
        else:
            have.append(t)
            out.append((SENSOR_MOVE, len(have) - 1))
    return out
