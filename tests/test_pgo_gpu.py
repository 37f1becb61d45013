"""GPU parity tests of the pose-graph half: HIP path (through the C ABI) vs the CPU oracle
(LM + sparse direct Cholesky, mirroring g2o + CSparse).  Tolerance from BASELINE.json's north_star:
pose error within 1e-3 m / 1e-4 rad after the same LM iteration count."""
import numpy as np
import pytest

from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu

TOL_T = 1e-3     # metres
TOL_R = 1e-4     # radians


@pytest.fixture(scope="module")
def pgo(capi):
    p = capi.Pgo()
    yield p
    p.close()


def _oracle_solve(oracle, g, iterations, xy=False, sensors=None):
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], sensors=sensors, optimize_xy_only=xy)
    fixed, n_gauge = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, st = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=iterations)
    return fl, fixed, n_gauge, P, st


def _check(pgo, oracle, g, iterations=20, xy=False, sensors=None, chi2_rtol=1e-6):
    pgo.set_config(optimize_xy_only=1 if xy else 0, iterations=iterations)
    pgo.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], sensors=sensors)
    st = pgo.optimize(iterations)
    poses, err, used = pgo.store()
    fl, fixed, n_gauge, P, so = _oracle_solve(oracle, g, iterations, xy, sensors)
    assert st["status"] == 0, st
    assert st["n_edges"] == len(fl["ij"]) and st["n_vertices"] == len(fixed)
    assert st["n_gauge_fixed"] == n_gauge
    assert np.array_equal(pgo.get_fixed(), fixed)
    assert np.array_equal(np.nonzero(used)[0], np.sort(fl["src_edge"]))
    # once LM has converged to round-off, whether rho is exactly 0 / slightly negative (Terminate) is noise:
    # the iteration counts must agree unless one side stopped early at the common fixed point
    if not (st["terminated_early"] or so["terminated_early"]):
        assert st["iterations_done"] == so["iterations_done"]
        # ... and the same accept / reject sequence (G7, g2o_optimizer.cpp:137-149): equal numbers of trials.  Not where the oracle itself says
        # a decision was rounding-level - a rejected trial (more trials than iterations) this close to convergence is one
        if so["lm_trials"] == so["iterations_done"]:
            assert st["lm_trials"] == so["lm_trials"], (st["lm_trials"], so["lm_trials"])
    assert abs(st["chi2_initial"] - so["chi2_initial"]) <= 1e-9 * abs(so["chi2_initial"]) + 1e-12
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    assert dt < TOL_T and dr < TOL_R, (dt, dr)
    assert abs(st["chi2_final"] - so["chi2_final"]) <= chi2_rtol * abs(so["chi2_final"]) + 1e-9
    # storeImpl edge errors (g2o_optimizer.cpp:124-131) on the solved poses
    want = oracle.edge_error_norms(P, fl["ij"], fl["meas"])
    got = err[fl["src_edge"]]
    assert np.allclose(got, want, atol=2e-4)
    assert np.isnan(err[used == 0]).all()
    return st, so


def test_c1_100_nodes_300_edges(pgo, oracle):
    """BASELINE config 1."""
    st, so = _check(pgo, oracle, synth.make_pose_graph(100, 300))
    assert st["lm_trials"] >= st["iterations_done"]


def test_c2_1k_nodes_5k_edges(pgo, oracle):
    """BASELINE config 2: 1k nodes / 5k edges, 20 LM iterations."""
    st, so = _check(pgo, oracle, synth.make_pose_graph(1000, 5000))
    assert st["iterations_done"] == 20


def test_xy_only(pgo, oracle):
    """optimize_xy_only = true is the deployed setting (iti_slam_launch/yaml/slam.yaml:50-53)."""
    _check(pgo, oracle, synth.make_pose_graph(300, 1200, seed=4), xy=True)


def test_chi2_of_first_iteration_matches(pgo, oracle):
    g = synth.make_pose_graph(200, 700, seed=9)
    pgo.set_config(optimize_xy_only=0, pcg_tol=1e-8)      # this test is about the first linearisation, not the solver tolerance
    pgo.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    st = pgo.optimize(1)
    fl, fixed, _, P, so = _oracle_solve(oracle, g, 1)
    assert abs(st["chi2_initial"] - so["chi2_initial"]) <= 1e-10 * so["chi2_initial"]
    poses, _, _ = pgo.store()
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    pgo.set_config(pcg_tol=1e-5)                  # back to the default for the tests that share this handle
    assert dt < 1e-5 and dr < 1e-6, (dt, dr)      # one LM step: only the PCG tolerance separates the two


def test_sensor_transforms_and_displacements(pgo, oracle):
    """Measurement composition disp_from * S_from * T * S_to^-1 * disp_to^-1 (g2o_optimizer.cpp:229,281)."""
    rng = np.random.default_rng(5)
    g = synth.make_pose_graph(150, 500, seed=6)
    E = len(g["edges"]["from"])

    def rand_T(k, scale):
        return synth.se3(synth.quat_to_R(synth.quat_from_rotvec(rng.normal(0, scale, (k, 3)))), rng.normal(0, scale, (k, 3)))

    sensors = rand_T(3, 0.2).reshape(-1, 12)
    g["edges"]["sensor_from"] = rng.integers(-1, 3, E).astype(np.int32)
    g["edges"]["sensor_to"] = rng.integers(-1, 3, E).astype(np.int32)
    # displacements: keep the composed measurement consistent by folding them into `transform`
    Df = rand_T(E, 0.05); Dt = rand_T(E, 0.05)
    T = g["edges"]["transform"].reshape(-1, 3, 4)
    I = np.tile(np.eye(3, 4), (4, 1, 1))
    S = np.concatenate([I[:1], sensors.reshape(-1, 3, 4)])     # index -1 -> identity
    Sf = S[g["edges"]["sensor_from"] + 1]; St = S[g["edges"]["sensor_to"] + 1]
    odom = g["edges"]["type"] == synth.EDGE_TYPE_ODOM
    # feature: Z = Df Sf T' St^-1 Dt^-1  =>  T' = Sf^-1 Df^-1 Z St Dt ; odometry: T' = Df^-1 Z Dt
    Tf = synth.se3_mul(synth.se3_mul(synth.se3_inv(Sf), synth.se3_inv(Df)), synth.se3_mul(synth.se3_mul(T, Dt), St))
    To = synth.se3_mul(synth.se3_inv(Df), synth.se3_mul(T, Dt))
    g["edges"]["transform"] = np.where(odom[:, None, None], To, Tf).reshape(-1, 12)
    g["edges"]["displacement_from"] = Df.reshape(-1, 12)
    g["edges"]["displacement_to"] = Dt.reshape(-1, 12)
    _check(pgo, oracle, g, sensors=sensors)


def test_gauge_fixing_of_disconnected_components(pgo, oracle):
    """setFixedNodes (g2o_optimizer.cpp:301-349): no fixed node at all, two components."""
    g1 = synth.make_pose_graph(60, 150, seed=1)
    g2 = synth.make_pose_graph(50, 120, seed=2)
    n1 = 60
    nodes = np.concatenate([g1["nodes_pose"], g2["nodes_pose"]])
    fixed = np.zeros(110, np.uint8)
    edges = {}
    for k in g1["edges"]:
        a, b = g1["edges"][k], g2["edges"][k]
        if k in ("from", "to"):
            b = b + n1
        edges[k] = np.concatenate([a, b])
    g = dict(nodes_pose=nodes, nodes_fixed=fixed, edges=edges)
    st, so = _check(pgo, oracle, g)
    assert st["n_gauge_fixed"] == 2
    f = pgo.get_fixed()
    assert f[0] == 1 and f[n1] == 1 and f.sum() == 2


def test_skip_rules_and_missing_nodes(pgo, oracle):
    g = synth.make_pose_graph(80, 240, seed=12)
    e = g["edges"]
    e["valid"][100:110] = 0                 # rejected by the TransformationFilter
    e["from"][120] = -1                     # endpoint missing from the graph (:77)
    e["to"][121] = 9999
    g["nodes_fixed"][10] = 1; g["nodes_fixed"][11] = 1   # odom 10->11 stays (both fixed), 11->12 dropped (:203-206)
    st, so = _check(pgo, oracle, g)


def test_set_graph_flat_entry(pgo, oracle):
    g = synth.make_pose_graph(120, 400, seed=3)
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    pgo.set_config(optimize_xy_only=0)
    pgo.set_graph(fl["poses"], fl["fixed"], fl["ij"], fl["meas"], fl["info"], fl["robust"])
    st = pgo.optimize(20)
    poses, err, used = pgo.store()
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, so = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=20)
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    assert dt < TOL_T and dr < TOL_R
    assert used.all()


def test_block_jacobi_and_multilevel_agree(capi, oracle):
    """The preconditioner only changes how fast PCG converges, never what it converges to."""
    g = synth.make_pose_graph(400, 1800, seed=21)
    out = []
    for pre in (0, 1):
        p = capi.Pgo(preconditioner=pre)
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        st = p.optimize(10)
        poses, _, _ = p.store()
        out.append((poses, st))
        p.close()
    dt, dr = synth.pose_errors(out[0][0].reshape(-1, 3, 4), out[1][0].reshape(-1, 3, 4))
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    assert out[1][1]["pcg_iterations"] < 0.5 * out[0][1]["pcg_iterations"], (out[0][1]["pcg_iterations"], out[1][1]["pcg_iterations"])
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, _ = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=10)
    for poses, _ in out:
        dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
        assert dt < TOL_T and dr < TOL_R


@pytest.mark.parametrize("n,e", [(9, 20), (17, 40), (64, 200), (65, 200), (513, 2000), (1281, 5000), (1800, 7000), (2049, 8000)])
def test_multilevel_hierarchy_edge_sizes(capi, oracle, n, e):
    """aggregate boundaries: 8^k and 8^k + 1 vertices, partially filled last aggregates; 1281 / 1800: the level-1 dense operator
    beyond 960 columns (ml_cg_comp_lm_kernel<8, ...>); 2049: the first size on the four-aggregates-per-workgroup path."""
    g = synth.make_pose_graph(n, e, seed=n)
    p = capi.Pgo()
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    st = p.optimize(8)
    poses, _, _ = p.store()
    p.close()
    assert st["status"] == 0
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, _ = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=8)
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    assert dt < TOL_T and dr < TOL_R, (dt, dr)


def test_large_graph_path_with_dense_level2_operator_matches_oracle(capi, oracle):
    """4000 free vertices: four aggregates per workgroup (gather level 2) with the hierarchy above level 2 folded into one dense
    operator (multiplicative cycle + Newton-Schulz on the f64 matrix cores), against the oracle's direct solve."""
    g = synth.make_pose_graph(4000, 16000, seed=40)
    p = capi.Pgo()
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    st = p.optimize(6)
    poses, _, _ = p.store()
    p.close()
    assert st["status"] == 0 and st["pcg_not_converged"] == 0
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, so = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=6)
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    assert dt < TOL_T and dr < TOL_R, (dt, dr)
    assert abs(st["chi2_final"] - so["chi2_final"]) <= 1e-4 * so["chi2_final"]
    # the exact level-2 solve halves the iteration count of the additive hierarchy (230 -> 110 per LM iteration at 10k vertices)
    assert st["pcg_iterations"] < 6 * 150


def test_dense_level2_operator_beyond_20k_vertices(capi):
    """30k vertices (6 n_2 = 5628: the dense level-2 operator's range since round 5, a 253-MB matrix): the CPU checker's direct solve of
    this size takes minutes, so the reference here is the SAME problem under the block-Jacobi preconditioner - another solver for the same
    linear systems - within the bar after the same LM iterations; and the operator must be what makes the solve short."""
    g = synth.make_pose_graph(30000, 150000, seed=8)
    res = {}
    for pre in (1, 0):
        p = capi.Pgo(preconditioner=pre)
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        st = p.optimize(5)
        res[pre] = (p.store()[0].reshape(-1, 3, 4), st)
        p.close()
        assert st["status"] == 0 and st["pcg_not_converged"] == 0
    dt, dr = synth.pose_errors(res[1][0], res[0][0])
    assert dt < TOL_T and dr < TOL_R, (dt, dr)
    assert res[1][1]["lm_trials"] == res[0][1]["lm_trials"]
    assert abs(res[1][1]["chi2_final"] - res[0][1]["chi2_final"]) <= 1e-6 * res[0][1]["chi2_final"]
    assert res[1][1]["pcg_iterations"] * 8 < res[0][1]["pcg_iterations"]


def test_degenerate_inputs(capi, pgo):
    pgo.set_config(optimize_xy_only=0)
    g = synth.make_pose_graph(20, 40, seed=8)
    # all vertices fixed: nothing to solve
    pgo.add_graph(g["nodes_pose"], np.ones(20, np.uint8), g["edges"])
    st = pgo.optimize(5)
    assert st["iterations_done"] == 0
    poses, _, _ = pgo.store()
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), g["nodes_pose"].reshape(-1, 3, 4))
    assert dt < 1e-12 and dr < 1e-7
    # no edges at all
    empty = {k: v[:0] for k, v in g["edges"].items()}
    pgo.add_graph(g["nodes_pose"], g["nodes_fixed"], empty)
    st = pgo.optimize(5)
    assert st["n_edges"] == 0
    # call order
    p2 = capi.Pgo()
    with pytest.raises(capi.UzlError) as e:
        p2.optimize(1)
    assert e.value.status == capi.UZL_ERR_STATE
    p2.close()


def test_use_odometry_parameters(capi, oracle):
    """GraphOptimizerConfig::use_odometry_parameters (g2o_optimizer.cpp:209-227): every odometry measurement goes through
    g2o's OdomConvert round trip before it is composed with the displacements."""
    g = synth.make_pose_graph(150, 500, seed=21)
    e = g["edges"]
    e["diff_time"][:149] = np.random.default_rng(1).uniform(0.1, 2.0, 149)
    e["diff_time"][7] = 0.0                                        # no elapsed time: the round trip yields zero motion
    e["diff_time"][9] = -0.8                                       # fabs() at :211
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], e, use_odometry_parameters=True)
    fl0 = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], e)
    assert np.abs(fl["meas"][:148] - fl0["meas"][:148]).max() > 1e-4          # the branch does something (lateral slip removed)
    assert np.array_equal(fl["meas"][148:], fl0["meas"][148:])                # feature edges untouched
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, so = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=8)
    p = capi.Pgo(use_odometry_parameters=1)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], e)
    st = p.optimize(8)
    poses, _, _ = p.store()
    p.close()
    assert abs(st["chi2_initial"] - so["chi2_initial"]) <= 1e-9 * so["chi2_initial"]
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    assert dt < 1e-3 and dr < 1e-4, (dt, dr)


def test_full_size_c4_vs_oracle_and_properties(pgo, oracle):
    """BASELINE config 4 size (10k nodes / 50k edges) on one GPU against the CPU checker's direct solve at full size (~20-35 s),
    bar 1e-3 m / 1e-4 rad after the same 20 LM iterations (G2oOptimizer::optimizeImpl, g2o_optimizer.cpp:137-149); then
    size-independent properties: chi2 decreases to a fixed point, re-optimising from the solution is idempotent, gauge untouched."""
    g = synth.make_pose_graph(10000, 50000)
    st, so = _check(pgo, oracle, g, iterations=20)
    assert st["status"] == 0 and st["iterations_done"] == 20
    assert st["chi2_final"] < 0.2 * st["chi2_initial"]
    poses, err, used = pgo.store()
    assert np.allclose(poses[0], g["nodes_pose"][0], atol=1e-12)
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), g["gt_pose"].reshape(-1, 3, 4))
    assert dt < 1.0
    # idempotence: start again from the optimum
    pgo.add_graph(poses, g["nodes_fixed"], g["edges"])
    st2 = pgo.optimize(3)
    assert abs(st2["chi2_final"] - st["chi2_final"]) <= 1e-6 * st["chi2_final"]
    poses2, _, _ = pgo.store()
    dt2, dr2 = synth.pose_errors(poses2.reshape(-1, 3, 4), poses.reshape(-1, 3, 4))
    assert dt2 < 1e-3 and dr2 < 1e-4


def test_rejected_trials_multi_edges_and_hub(capi, oracle):
    """LM trials that get rejected (lambda grows, same linearisation is solved again), several edges between the same two
    nodes (their blocks add up in the block-CSR and in the sibling blocks) and a hub vertex with far more than ten slots."""
    g = synth.make_pose_graph(240, 900, seed=77, outlier_frac=0.35)
    e = g["edges"]
    rng = np.random.default_rng(5)
    # poor initial guess: scramble the dead-reckoning poses (rotations too: that is what makes LM reject steps)
    P0 = g["nodes_pose"].reshape(-1, 3, 4).copy()
    P0[1:] = synth.se3_mul(P0[1:], synth.se3_from_noise(rng.normal(0, 1.5, (239, 3)), rng.normal(0, 0.8, (239, 3))))
    # multi-edges: duplicate 40 loop closures (same endpoints, same measurement)
    dup = np.arange(300, 340)
    # hub: 60 extra loop closures from node 100 to nodes 101..160 built from the ground truth
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
    fl = oracle.flatten_graph(P0.reshape(-1, 12), g["nodes_fixed"], e2)
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    its = 8
    P, so = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=its)
    # this far from the optimum the LM path is chaotic (a solve error grows ~10x per iteration, measured): solve tightly
    p = capi.Pgo(pcg_tol=1e-12)
    p.add_graph(P0.reshape(-1, 12), g["nodes_fixed"], e2)
    st = p.optimize(its)
    poses, _, _ = p.store()
    p.close()
    assert so["lm_trials"] > so["iterations_done"] + 3, "the case is meant to contain rejected trials"
    assert st["pcg_not_converged"] == 0
    assert st["lm_trials"] == so["lm_trials"] and st["iterations_done"] == so["iterations_done"]
    assert abs(st["chi2_final"] - so["chi2_final"]) <= 1e-6 * so["chi2_final"]
    dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
    assert dt < 1e-3 and dr < 1e-4, (dt, dr)


@pytest.mark.parametrize("n", [16, 64, 100, 750, 959, 1006, 1878])
def test_ns_gemm_matrix_core_layout(capi, n):
    """the f64 MFMA tile kernel of the Newton-Schulz refinement (X' = 2 X - X T) against numpy, including edge tiles.  The kernel
    computes the tiles on and above the diagonal and mirrors them (X, A and X A X are symmetric in the refinement)."""
    import ctypes
    rng = np.random.default_rng(n)
    f64p = ctypes.POINTER(ctypes.c_double)

    def run(X, T):
        out = np.zeros((n, n))
        rc = capi.diag_lib().uzl_debug_ns_gemm(ctypes.c_int(n), np.ascontiguousarray(X).ctypes.data_as(f64p), np.ascontiguousarray(T).ctypes.data_as(f64p),
                                          out.ctypes.data_as(f64p))
        assert rc == 0
        return out

    # arbitrary operands: the X tile of the product is read through X's symmetry (as X[k][row]), so upper tiles = 2 X - X^T T,
    # lower tiles = their mirror images ("tiles" of 32: inside a 64 x 64 tile on the diagonal the quarter below the diagonal is a mirror
    # image too, as in the 32 x 32 tiling of the small-graph kernel)
    X = rng.normal(size=(n, n)); T = rng.normal(size=(n, n))
    full = 2 * X - X.T @ T
    t32 = np.arange(n) // 32
    upper = t32[:, None] <= t32[None, :]
    want = np.where(upper, full, full.T)
    out = run(X, T)
    assert np.abs(out - want).max() <= 1e-11 * np.abs(want).max()
    # the refinement's operands: X symmetric, T = A X with A symmetric -> the whole matrix, symmetric to the last bit off the diagonal tiles
    A = rng.normal(size=(n, n)); A = A + A.T
    X = rng.normal(size=(n, n)); X = X + X.T
    out = run(X, A @ X)
    want = 2 * X - X @ A @ X
    assert np.abs(out - want).max() <= 1e-10 * np.abs(want).max()
    off = t32[:, None] != t32[None, :]
    assert np.array_equal(out[off], out.T[off])
    # the small-graph kernel (32 x 32 tiles, K split over the four waves): the same sums in the same order - the same bits wherever both
    # kernels compute the entry themselves (tiles on and above the diagonal of BOTH tilings; the rest are mirror images)
    if n > 960:          # (kGemm32Max: beyond it only the 64 x 64 kernel runs - 1006: edge tiles with a partial last slab; 1878: config 4's size)
        return
    out32 = np.zeros((n, n))
    rc = capi.diag_lib().uzl_debug_ns_gemm32(ctypes.c_int(n), np.ascontiguousarray(X).ctypes.data_as(f64p), np.ascontiguousarray(A @ X).ctypes.data_as(f64p),
                                        out32.ctypes.data_as(f64p))
    assert rc == 0
    assert np.abs(out32 - want).max() <= 1e-10 * np.abs(want).max()
    assert np.array_equal(out32, out)
    assert np.array_equal(out32[off], out32.T[off])


def test_handles_driven_from_concurrent_threads(capi):
    """One handle per host thread (the reference runs each plugin on its own worker thread, graph_optimizer.cpp:35-73,
    transformation_estimator.cpp:22-62): concurrent solves and match batches give exactly what the same calls give one after the other."""
    import threading
    graphs = [synth.make_pose_graph(n, e, seed=s) for n, e, s in ((300, 1200, 1), (900, 4000, 2), (1500, 6000, 3), (2600, 10000, 4))]
    pairs = synth.make_pairs(24, n_kp=400, seed=8)

    def solve(g):
        p = capi.Pgo()
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        out = []
        for _ in range(2):
            p.reset(); st = p.optimize(6); out.append((st["status"], st["chi2_final"], p.store()[0].copy()))
        p.close()
        return out

    def match():
        m = capi.Match(ransac_threshold=0.1, ransac_iteration=200, ransac_break_percentage=0.6, seed=3)
        ids = [(m.add_frame(f["desc"], f["pos"], f["valid"]), m.add_frame(t["desc"], t["pos"], t["valid"])) for f, t, _ in pairs]
        res = [m.estimate(ids)[0] for _ in range(3)]
        m.close()
        return [(r["consensus"], r["T"].copy()) for r in res[-1]]

    ref = [solve(g) for g in graphs] + [match(), match()]
    got = [None] * 6
    def run(i):
        got[i] = solve(graphs[i]) if i < 4 else match()
    th = [threading.Thread(target=run, args=(i,)) for i in range(6)]
    for t in th: t.start()
    for t in th: t.join()
    for i in range(4):
        for (s0, c0, p0), (s1, c1, p1) in zip(ref[i], got[i]):
            assert s0 == s1 == 0 and c0 == c1 and np.array_equal(p0, p1)
    for i in (4, 5):
        for (c0, T0), (c1, T1) in zip(ref[i], got[i]):
            assert c0 == c1 and np.array_equal(T0, T1)


@pytest.mark.parametrize("n,e,its", [(3000, 3100, 10), (8000, 8400, 10), (2000, 2040, 10), (1500, 1530, 20)])
def test_chain_like_graphs(capi, oracle, n, e, its):
    """Few loop closures per vertex - the shape a graph has during an online run (BASELINE config 5).  On these the
    multiplicative cycle / Newton-Schulz operator of the composite preconditioner loses positive definiteness once lambda
    has come down (round 1 returned `converged` on r.z < 0 here: 4.5 m off the direct solve).  The solver must notice
    (negative r.M^-1 r is a breakdown, the true residual is checked) and finish with the additive operator."""
    p = capi.Pgo()
    try:
        st, so = _check(p, oracle, synth.make_pose_graph(n, e), iterations=its)
        assert st["pcg_not_converged"] == 0
        # the handle remembers: the next structure starts with the additive operator and still agrees with the oracle
        _check(p, oracle, synth.make_pose_graph(n // 2, e // 2 + 20, seed=5), iterations=its)
    finally:
        p.close()


@pytest.mark.parametrize("n,e", [(10000, 10800), (12600, 13600), (20000, 21700), (23000, 24600)])
def test_large_sparse_graphs_on_every_kernel_path_against_oracle(capi, oracle, n, e):
    """The large-graph PCG kernels against the oracle's direct solve at sizes the oracle still finishes in a second (few loop closures:
    little fill): 10k = six rows of the level-2 operator in registers (ml_cg_lm_kernel<4, true, true, ...>), 12.6k and 20k = ml_alpha_lm_kernel +
    streamed rows (ml_cg_lm_kernel<4, true, false, true, ...>; 6 n_2 = 2364 / 3750), 23k = no dense level-2 operator (6 n_2 > 4096:
    ml_cg_lm_kernel<4, false, ...>, restrict / top solve / prolong through LDS); ml_spmv_lm_kernel<4, ...> in half-aggregate workgroups throughout."""
    p = capi.Pgo()
    try:
        st, so = _check(p, oracle, synth.make_pose_graph(n, e, seed=n), iterations=6)
        assert st["pcg_not_converged"] == 0
    finally:
        p.close()


def test_near_tree_graph_without_odometry(capi, oracle):
    """A graph whose odometry chain is gone and whose loop closures barely connect it (3500 vertices, 3501 system edges): beam-like, the
    preconditioned system is badly conditioned (1900 PCG iterations per solve) and a relative residual tolerance that is fine elsewhere
    left 2.9e-3 m / 1.3e-4 rad against the direct solve (tests/diag/stress_pgo.py seed 21, case 5).  The solve now stops on an estimate
    of the error left in the step itself, in metres / radians (csrc/pgo_device.hpp: progress_decide_ml)."""
    g = synth.drop_odometry(synth.make_pose_graph(3500, 7000, seed=779627, outlier_frac=0.2), keep_every=0)
    p = capi.Pgo()
    try:
        st, so = _check(p, oracle, g, iterations=8)
        assert st["pcg_not_converged"] == 0
    finally:
        p.close()


def test_vertex_order_does_not_matter(capi, oracle):
    """The aggregates of the preconditioner are 8 consecutive blocks of an order derived from the graph (heaviest-edge chains,
    pgo_structure.hip aggregation_order), not of the node index: renumbered nodes, two sessions with interleaved ids (merged / global-scope
    graphs, graph_slam_node.cpp:401-576) and graphs without an odometry chain must solve to the oracle's result with iteration
    counts close to the time-ordered case (with index-order aggregates they were 7x / 4-6x higher)."""
    n, e, its = 1000, 5000, 10
    g = synth.make_pose_graph(n, e)
    p = capi.Pgo()
    try:
        st_nat, _ = _check(p, oracle, g, iterations=its)
        rng = np.random.default_rng(1)
        perm = rng.permutation(n)
        st_perm, _ = _check(p, oracle, synth.permute_graph(g, perm), iterations=its)
        st_rev, _ = _check(p, oracle, synth.permute_graph(g, np.arange(n)[::-1].copy()), iterations=its)
        st_two, _ = _check(p, oracle, synth.interleave_sessions(synth.make_pose_graph(n // 2, e // 2, seed=1), synth.make_pose_graph(n // 2, e // 2, seed=2)),
                           iterations=its)
        base = st_nat["pcg_iterations"]
        assert st_perm["pcg_iterations"] <= 1.25 * base and st_rev["pcg_iterations"] <= 1.25 * base and st_two["pcg_iterations"] <= 1.5 * base, \
            (base, st_perm["pcg_iterations"], st_rev["pcg_iterations"], st_two["pcg_iterations"])
        # the permuted solve is the SAME problem: same chi2 trajectory end point, poses equal after un-permuting
        p.add_graph(**{k: v for k, v in zip(("nodes_pose", "nodes_fixed", "edges"), (g["nodes_pose"], g["nodes_fixed"], g["edges"]))})
        p.optimize(its); P0 = p.store()[0]
        gp = synth.permute_graph(g, perm)
        p.add_graph(gp["nodes_pose"], gp["nodes_fixed"], gp["edges"])
        p.optimize(its); P1 = p.store()[0]
        dt, dr = synth.pose_errors(P1[perm].reshape(-1, 3, 4), P0.reshape(-1, 3, 4))
        assert dt < 1e-4 and dr < 1e-5, (dt, dr)
        # no odometry chain at all / a broken one: harder systems (weaker coupling), still the oracle's answer, bounded iteration counts
        st_no, _ = _check(p, oracle, synth.drop_odometry(g), iterations=20)
        st_5, _ = _check(p, oracle, synth.drop_odometry(g, keep_every=5), iterations=20)
        assert st_no["n_gauge_fixed"] > 0                                    # components without a fixed node got their gauge
        assert st_no["pcg_iterations"] / st_no["lm_trials"] < 200 and st_5["pcg_iterations"] / st_5["lm_trials"] < 320, \
            (st_no["pcg_iterations"], st_no["lm_trials"], st_5["pcg_iterations"], st_5["lm_trials"])
    finally:
        p.close()


def test_20k_nodes_100k_edges_properties(capi):
    """The largest graph the dense level-2 operator serves (BASELINE config 5's node count with config 4's edge density).  The
    oracle's direct solve would take minutes; checked through properties: LM only descends, the solve is reproducible bit for
    bit, a solve at a 100x tighter PCG tolerance lands within the parity bar of the default one, the map beats dead reckoning."""
    g = synth.make_pose_graph(20000, 100000)
    out = []
    for tol in (1e-5, 1e-5, 1e-7):
        p = capi.Pgo(pcg_tol=tol)
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        st = p.optimize(20)
        out.append((st, p.store()[0]))
        p.close()
    (s0, P0), (s1, P1), (s2, P2) = out
    assert s0["status"] == 0 and s0["iterations_done"] == 20 and s0["pcg_not_converged"] == 0
    assert s0["chi2_final"] < 0.2 * s0["chi2_initial"]
    assert np.array_equal(P0, P1) and s0["pcg_iterations"] == s1["pcg_iterations"]
    dt, dr = synth.pose_errors(P0.reshape(-1, 3, 4), P2.reshape(-1, 3, 4))
    assert dt < 1e-3 and dr < 1e-4, (dt, dr)
    gt = g["gt_pose"].reshape(-1, 3, 4)
    e0 = np.linalg.norm(g["nodes_pose"].reshape(-1, 3, 4)[:, :, 3] - gt[:, :, 3], axis=1).mean()
    e1 = np.linalg.norm(P0.reshape(-1, 3, 4)[:, :, 3] - gt[:, :, 3], axis=1).mean()
    assert e1 < 0.1 * e0, (e0, e1)


def test_structure_is_kept_when_only_values_change(capi, oracle):
    """A re-optimisation of a graph whose vertices, fixed flags, system edges and edge weights did not change (the timer-driven
    optimize() of graph_slam_node.cpp:1138-1150 on an unchanged or merely moved graph) keeps gauge, block-CSR, hierarchy arrays and
    the captured PCG graph; any structural change rebuilds.  Either way the result is the one a fresh handle computes."""
    g = synth.make_pose_graph(1200, 5000, seed=21)
    p = capi.Pgo()
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    s1 = p.optimize(6)
    assert s1["structure_reused"] == 0 and s1["structure_ms"] > 0
    # same topology, moved poses and measurements
    g2 = dict(g); g2["nodes_pose"] = p.store()[0]
    e2 = {k: np.array(v) for k, v in g["edges"].items()}
    e2["transform"] = e2["transform"] + 1e-3 * np.random.default_rng(0).normal(size=e2["transform"].shape) * (np.arange(12) % 4 == 3)
    g2["edges"] = e2
    p.add_graph(g2["nodes_pose"], g2["nodes_fixed"], g2["edges"])
    s2 = p.optimize(6)
    assert s2["structure_reused"] == 1 and s2["structure_ms"] < 0.25 * s1["structure_ms"]
    fresh = capi.Pgo()
    fresh.add_graph(g2["nodes_pose"], g2["nodes_fixed"], g2["edges"])
    sf = fresh.optimize(6)
    assert np.array_equal(p.store()[0], fresh.store()[0]) and s2["pcg_iterations"] == sf["pcg_iterations"]
    _check(fresh, oracle, g2, iterations=6)
    # one edge fewer: rebuilt
    e3 = {k: np.asarray(v)[:-1] for k, v in e2.items()}
    p.add_graph(g2["nodes_pose"], g2["nodes_fixed"], e3)
    s3 = p.optimize(3)
    assert s3["structure_reused"] == 0 and s3["n_edges"] == s2["n_edges"] - 1
    # the same last edge present but not valid (TransformationFilter verdict): the SAME system as without it - kept
    e4 = {k: np.array(v) for k, v in e2.items()}
    e4["valid"][-1] = 0
    p.add_graph(g2["nodes_pose"], g2["nodes_fixed"], e4)
    assert p.optimize(3)["structure_reused"] == 1
    # another edge loses its verdict: rebuilt
    e4["valid"][-2] = 0
    p.add_graph(g2["nodes_pose"], g2["nodes_fixed"], e4)
    assert p.optimize(3)["structure_reused"] == 0
    p.close(); fresh.close()


def test_random_shapes_against_oracle():
    """Randomized sweep (tests/diag/stress_pgo.py): sizes 150 .. 5000, 1.01 .. 5 edges per node, 0 - 20 % outliers, natural / renumbered /
    broken odometry chain, xy-only or not, 3 / 8 / 15 LM iterations - every case within the north-star tolerance of the oracle's
    direct solve after the same iteration count.  Seed 11 is the sweep on which a fixed relative 1e-5 PCG tolerance left two sparse-loop
    graphs 1.2e-4 / 1.7e-4 rad off after 3 iterations (large first steps): the stop test is now on the step's error, not the residual."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "diag", "stress_pgo.py"), "110", "11"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "110 cases, 0 misses" in r.stdout


def test_pcg_cap_and_accuracy_settings(capi, oracle):
    """The replay policy (short and long captured graphs, the stop test inside the iteration kernels) at its edges: a cap of a few PCG
    iterations ends every solve at the cap and says so; a looser / tighter `pcg_tol` moves the iteration count the right way and both
    stay inside the north-star tolerance of the CPU checker's direct solve; pcg_tol = 0 (no accuracy target: the relative floor is
    zero as well) iterates every solve to the cap."""
    g = synth.make_pose_graph(600, 2400, seed=31)
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, _ = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=10)

    def solve(**cfg):
        p = capi.Pgo(**cfg)
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        st = p.optimize(10)
        poses = p.store()[0]
        p.close()
        return st, synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))

    st, _ = solve(pcg_max_iter=3)
    assert st["status"] == capi.UZL_ERR_NOT_CONVERGED and st["pcg_not_converged"] == st["lm_trials"] > 0
    # (the cap is checked between replays of 4 iterations, and a solve that did not converge is retried with fresh inverses / the additive operator)
    assert 3 * st["lm_trials"] <= st["pcg_iterations"] <= 12 * st["lm_trials"]
    base, (dt, dr) = solve()
    assert base["status"] == 0 and dt < 1e-3 and dr < 1e-4
    loose, (dtl, drl) = solve(pcg_tol=1e-4)
    tight, (dtt, drt) = solve(pcg_tol=1e-7)
    assert loose["pcg_iterations"] < base["pcg_iterations"] < tight["pcg_iterations"]
    assert dtl < 1e-3 and drl < 1e-4 and dtt < 1e-3 and drt < 1e-4 and dtt <= dt * 1.5 + 1e-9
    cap = 40
    full, _ = solve(pcg_tol=0.0, pcg_max_iter=cap)
    assert full["pcg_iterations"] >= cap * full["lm_trials"]


def test_ill_conditioned_long_chain_one_far_closure(capi, oracle):
    """the step-error stop test extrapolates from how far x moved in the last two PCG iterations; CG is not monotone and can
    sit almost still on a stiff system while far from the solution.  A 4000-vertex odometry chain closed by ONE loop closure between its
    ends, started from dead reckoning that has drifted by metres: the softest mode (the whole chain bending) carries the step.  Both stop
    tests - the default and cfg.pcg_stop = 1 (the plain relative residual test) - must stay within the bar of the direct solve."""
    g = synth.make_pose_graph(4000, 4000, seed=31, outlier_frac=0.0)          # 3999 odometry edges + 1 loop closure
    e = {k: np.asarray(v).copy() for k, v in g["edges"].items()}
    gt = g["gt_pose"].reshape(-1, 3, 4)
    k = len(e["from"]) - 1
    e["from"][k] = 3; e["to"][k] = 3990
    e["transform"][k] = synth.se3_mul(synth.se3_inv(gt[3:4]), gt[3990:3991]).reshape(12)
    g["edges"] = e
    for cfg in (dict(), dict(pcg_stop=1, pcg_tol=1e-7), dict(schur_reduce=-1)):
        p = capi.Pgo(**cfg)
        try:
            st, so = _check(p, oracle, g, iterations=6, chi2_rtol=1e-5)      # (six iterations from metres of drift: chi2 still falls by 1e-6 per step)
            assert st["pcg_not_converged"] == 0
        finally:
            p.close()



@pytest.mark.parametrize("n,e", [(6000, 6500), (20000, 21700)])
def test_reduced_numbering_row_order_and_strong_aggregates_agree(capi, oracle, n, e):
    """uzl_pgo_cfg::reduced_numbering: the Schur-reduced system in row order (1) and numbered by strong aggregates with empty rows (2) is the
    same linear system - same LM trajectory within the PCG's accuracy, both within the bar of the oracle's direct solve; 0 lets the handle
    choose (by the shape of the groups at first)."""
    g = synth.make_pose_graph(n, e, seed=n + 3)
    out = {}
    for mode in (1, 2, 0):
        p = capi.Pgo(reduced_numbering=mode)
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        st = p.optimize(8)
        out[mode] = (p.store()[0].reshape(-1, 3, 4), st)
        p.close()
        assert st["status"] == 0 and st["n_eliminated"] > n // 2
    for mode in (2, 0):
        a, b = out[1][1], out[mode][1]
        assert (a["iterations_done"], a["lm_trials"], a["n_eliminated"]) == (b["iterations_done"], b["lm_trials"], b["n_eliminated"])
        assert abs(a["chi2_final"] - b["chi2_final"]) <= 1e-6 * a["chi2_final"]
        dt, dr = synth.pose_errors(out[1][0], out[mode][0])
        assert dt < 1e-4 and dr < 1e-5, (mode, dt, dr)
    assert out[1][1]["pcg_iterations"] != out[2][1]["pcg_iterations"]          # (they ARE different preconditioners)
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    P, _ = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=8)
    for mode in (1, 2):
        dt, dr = synth.pose_errors(out[mode][0], P.reshape(-1, 3, 4))
        assert dt < 1e-3 and dr < 1e-4, (mode, dt, dr)


def test_blocks_with_hundreds_of_contributions(capi, oracle):
    """ml_galerkin_kernel's passes: one coarse block with more contributions than a workgroup transforms at once - 400 parallel edges
    between two vertices of DIFFERENT aggregates (an off-diagonal block of level 1) and 300 between two vertices of the SAME aggregate (a
    diagonal block) - plus the ordinary chunks around them.  Against the oracle."""
    g = synth.make_pose_graph(300, 900, seed=41)
    e = g["edges"]
    gt = g["gt_pose"].reshape(-1, 3, 4)
    rng = np.random.default_rng(9)

    def bundle(a, b, count):
        T = synth.se3_mul(synth.se3_inv(gt[[a] * count]), gt[[b] * count])
        T = synth.se3_mul(T, synth.se3_from_noise(rng.normal(0, 0.01, (count, 3)), rng.normal(0, 0.002, (count, 3))))
        return np.full(count, a, np.int32), np.full(count, b, np.int32), T.reshape(-1, 12)
    fa, ta, Ta = bundle(40, 170, 400)
    fb, tb, Tb = bundle(80, 81, 300)
    nx = 700
    ident = np.tile(np.eye(3, 4).reshape(1, 12), (nx, 1))
    info = np.tile((np.eye(6) * 20.0).reshape(1, 36), (nx, 1))

    def cat(k, extra):
        return np.concatenate([np.asarray(e[k]), extra])
    e2 = {"from": cat("from", np.concatenate([fa, fb])), "to": cat("to", np.concatenate([ta, tb])),
          "type": cat("type", np.ones(nx, np.int32)), "sensor_from": cat("sensor_from", np.full(nx, -1, np.int32)),
          "sensor_to": cat("sensor_to", np.full(nx, -1, np.int32)), "valid": cat("valid", np.ones(nx, np.int32)),
          "transform": cat("transform", np.concatenate([Ta, Tb])), "displacement_from": cat("displacement_from", ident),
          "displacement_to": cat("displacement_to", ident), "information": cat("information", info),
          "diff_time": cat("diff_time", np.zeros(nx))}
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], e2)
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    its = 8
    P, so = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=its)
    for loop in (0, 1):
        p = capi.Pgo(lm_loop=loop)
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], e2)
        st = p.optimize(its)
        poses, _, _ = p.store()
        p.close()
        assert st["status"] == 0 and st["iterations_done"] == so["iterations_done"]
        dt, dr = synth.pose_errors(poses.reshape(-1, 3, 4), P.reshape(-1, 3, 4))
        assert dt < 1e-3 and dr < 1e-4, (loop, dt, dr)
