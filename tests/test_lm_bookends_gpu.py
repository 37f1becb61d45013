"""The bookends of a one-graph pass of the device-resident LM loop: the PCG init of the small-graph class (x = 0, r = b, the exact
gather-level residual) goes out as further workgroups of the head's launch (lm_head_init_pcg_kernel, csrc/pgo_ml_kernels.hip) where the
pass has no synchronous set-up and the system is not Schur-reduced (lm_init_rides, csrc/pgo_lm_pass.hpp), and the head clears the
solve's flags itself.  Existing arithmetic in another launch: the device-resident loop must give the host-driven loop's bits - poses,
edge errors, chi2, lambda, every counter - and a batch the single solve's, on graphs of one and of several init workgroups, with
rejected trials and a set-up retake (passes that keep the separate init), at the PCG cap (the anomaly path), in the plane, and on a
chain-like graph whose reduced system keeps the old pass shape.  The host enqueues the passes it enqueued before (PARENT_PASSES: what
the parent commit's library gives on the same graphs)."""
import numpy as np
import pytest

from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ("status", "iterations_done", "lm_trials", "pcg_iterations", "pcg_not_converged", "terminated_early", "precond_builds",
        "n_eliminated", "chi2_initial", "chi2_final", "lambda_final")

# lm_passes of the first optimize of every case below with the parent commit's library
# ("cap": the host-driven loop took the graph over, and the stats are its own)
PARENT_PASSES = {"24/60": 8, "64/200": 8, "200/1000": 10, "rejected": 48, "cap": 0, "xy": 10, "chain": 13}


def _solve(capi, g, its, loop, **cfg):
    p = capi.Pgo(lm_loop=loop, **cfg)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    st = p.optimize(its)
    poses, err, _ = p.store()
    st2 = p.optimize(2)                           # a second optimize on the same handle continues from the result
    poses2, _, _ = p.store()
    p.close()
    return st, poses, err, st2, poses2


def _same(capi, name, g, its, **cfg):
    a = _solve(capi, g, its, 0, **cfg)
    b = _solve(capi, g, its, 1, **cfg)
    print(name, "lm_passes", a[0]["lm_passes"], {k: a[0][k] for k in KEYS})
    for st_a, st_b in ((a[0], b[0]), (a[3], b[3])):
        for k in KEYS:
            assert st_a[k] == st_b[k], (k, st_a, st_b)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])
    assert np.array_equal(a[2], b[2], equal_nan=True)
    assert b[0]["lm_passes"] == 0
    assert a[0]["lm_passes"] == PARENT_PASSES[name], (name, a[0]["lm_passes"])
    return a[0]


def _rejected_scene():
    """tests/test_pgo_gpu.py::test_rejected_trials_multi_edges_and_hub: a scrambled start (rejected trials, lambda grown 32x: a set-up
    retake), duplicated loop closures and a hub vertex"""
    g = synth.make_pose_graph(240, 900, seed=77, outlier_frac=0.35)
    e = g["edges"]
    rng = np.random.default_rng(5)
    P0 = g["nodes_pose"].reshape(-1, 3, 4).copy()
    P0[1:] = synth.se3_mul(P0[1:], synth.se3_from_noise(rng.normal(0, 1.5, (239, 3)), rng.normal(0, 0.8, (239, 3))))
    dup = np.arange(300, 340)
    gt = g["gt_pose"].reshape(-1, 3, 4)
    hub_to = np.arange(101, 161)
    hub_T = synth.se3_mul(synth.se3_inv(gt[[100] * 60]), gt[hub_to]).reshape(-1, 12)

    def cat(k, extra):
        return np.concatenate([np.asarray(e[k]), np.asarray(e[k])[dup], extra])

    ident = np.tile(np.eye(3, 4).reshape(1, 12), (60, 1))
    info = np.tile((np.eye(6) * 50.0).reshape(1, 36), (60, 1))
    e2 = {"from": cat("from", np.full(60, 100, np.int32)), "to": cat("to", hub_to.astype(np.int32)),
          "type": cat("type", np.ones(60, np.int32)), "sensor_from": cat("sensor_from", np.full(60, -1, np.int32)),
          "sensor_to": cat("sensor_to", np.full(60, -1, np.int32)), "valid": cat("valid", np.ones(60, np.int32)),
          "transform": cat("transform", hub_T), "displacement_from": cat("displacement_from", ident),
          "displacement_to": cat("displacement_to", ident), "information": cat("information", info),
          "diff_time": cat("diff_time", np.zeros(60))}
    return dict(g, nodes_pose=P0.reshape(-1, 12), edges=e2)


@pytest.mark.parametrize("n,e", [(24, 60), (64, 200), (200, 1000)])
def test_init_in_the_heads_launch_gives_the_host_loops_bits(capi, n, e):
    """3, 8 and 25 init workgroups behind the head's (8 vertices each; 24 and 200: the last one partly filled)"""
    st = _same(capi, "%d/%d" % (n, e), synth.make_pose_graph(n, e, seed=n + e), 8)
    assert st["status"] == 0 and st["n_eliminated"] == 0 and st["iterations_done"] >= 1


def test_rejected_trials_and_a_setup_retake(capi):
    """kLmRetry passes carry the init in the head's launch; the pass that retakes the inverses keeps the separate one"""
    st = _same(capi, "rejected", _rejected_scene(), 8, pcg_tol=1e-12)
    assert st["lm_trials"] > st["iterations_done"] + 3, "the case is meant to contain rejected trials"


def test_at_the_pcg_cap_the_anomaly_path_runs(capi):
    """a solve that ends at its cap is an anomaly of the device-resident loop: the host-driven loop takes the graph over"""
    st = _same(capi, "cap", synth.make_pose_graph(200, 1000, seed=1200), 6, pcg_max_iter=3)
    assert st["status"] == capi.UZL_ERR_NOT_CONVERGED and st["pcg_not_converged"] == st["lm_trials"] > 0


def test_optimize_xy_only(capi):
    _same(capi, "xy", synth.make_pose_graph(200, 1000, seed=1200), 8, optimize_xy_only=1)


def test_a_schur_reduced_system_keeps_the_separate_init(capi):
    st = _same(capi, "chain", synth.make_pose_graph(1500, 1530, seed=3), 10)
    assert st["n_eliminated"] > 0


def test_batch_gives_the_single_solves_bits(capi):
    """the batch's kernels keep the launch sequence they had: the reference of the one-graph pass"""
    graphs = [synth.make_pose_graph(200, 1000, seed=1200 + k) for k in range(3)]
    bt = capi.PgoBatch(len(graphs))
    for k, g in enumerate(graphs):
        bt.graphs[k].add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    stats = bt.optimize(8)
    assert bt.n_batched == len(graphs)
    for k, g in enumerate(graphs):
        p = capi.Pgo()
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        st = p.optimize(8)
        poses, err, _ = p.store()
        p.close()
        bp, be, _ = bt.graphs[k].store()
        assert np.array_equal(bp, poses) and np.array_equal(be, err, equal_nan=True), k
        for f in ("iterations_done", "lm_trials", "pcg_iterations", "precond_builds", "terminated_early", "chi2_initial", "chi2_final", "lambda_final"):
            assert stats[k][f] == st[f], (k, f, stats[k][f], st[f])
    bt.close()
