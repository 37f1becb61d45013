"""The solves whose pass counts tests/golden/lm_pass_counts.json pins (tests/test_lm_pass_counts_gpu.py, recorded by
tests/golden/make_lm_pass_counts.py): one function per case, each returning the list of per-optimize records it produced.
What the host predicts for a pass (csrc/pgo_lm_pass.hpp) never changes a result - only how many passes a solve takes - so the record of
an optimize is its pass count beside the counters that say the solve itself was the same."""
import numpy as np

from uzliti_slam_amd import synth

FIELDS = ("lm_passes", "lm_trials", "pcg_iterations", "iterations_done")


def _rec(st):
    return {k: int(st[k]) for k in FIELDS}


def _one(capi, g, its, **cfg):
    p = capi.Pgo(**cfg)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    out = [_rec(p.optimize(its))]
    p.close()
    return out


def _history(capi, hist):
    """three optimizes of one handle with reset() in between: the second and third size their passes from the one before (pass_history 0)"""
    g = synth.make_pose_graph(100, 300)
    p = capi.Pgo(pass_history=hist)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    out = []
    for k in range(3):
        if k:
            p.reset()
        out.append(_rec(p.optimize(12)))
    p.close()
    return out


def _batch(capi):
    """five graphs through two slots: cohorts of 2, 2 and 1 - the last with an idle slot beside it"""
    graphs = [synth.make_pose_graph(100, 300, seed=s) for s in range(1, 6)]
    bt = capi.PgoBatch(len(graphs))
    for k, g in enumerate(graphs):
        bt.graphs[k].add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    bt.set_resident(2)
    stats = bt.optimize(10)
    assert bt.n_batched == len(graphs)
    bt.close()
    return [_rec(st) for st in stats]


def scrambled_graph():
    """the scrambled-start graph of test_lm_loops_gpu.test_rejected_trials_and_termination: rejected trials, the 32x retake"""
    g = synth.make_pose_graph(240, 900, seed=77, outlier_frac=0.35)
    rng = np.random.default_rng(5)
    P0 = g["nodes_pose"].reshape(-1, 3, 4).copy()
    P0[1:] = synth.se3_mul(P0[1:], synth.se3_from_noise(rng.normal(0, 1.5, (239, 3)), rng.normal(0, 0.8, (239, 3))))
    g2 = dict(g); g2["nodes_pose"] = P0.reshape(-1, 12)
    return g2


CASES = {
    "1 64/70 5 its": lambda capi: _one(capi, synth.make_pose_graph(64, 70), 5),
    "2 100/300 20 its": lambda capi: _one(capi, synth.make_pose_graph(100, 300), 20),
    "3 300/1200 7 its": lambda capi: _one(capi, synth.make_pose_graph(300, 1200), 7),
    "4 1500/1530 Schur-reduced 10 its": lambda capi: _one(capi, synth.make_pose_graph(1500, 1530, seed=3), 10),
    "5 100/300 3 x 12 its pass_history 0": lambda capi: _history(capi, 0),
    "5 100/300 3 x 12 its pass_history 1": lambda capi: _history(capi, 1),
    "6 batch 5 x 100/300 resident 2": _batch,
    "7 240/900 scrambled start 8 its": lambda capi: _one(capi, scrambled_graph(), 8, pcg_tol=1e-12),
}
