"""The geometry of the pose-graph solve on the device, at 3-D rotations and at the edges of its branches: quat_from_R, pose_from_T,
project_xy, odom_round_trip (csrc/pgo_device.hpp), prepare_nodes / prepare_edges, edge_geom_of / edge_geom_rec with the w < 0 flip,
retract_pose and its inlined copies, and the Jacobians of hessian_rows_body (csrc/pgo_kernels.hip).  Every other device test of this
code draws a planar trajectory (synth.make_pose_graph: roll and pitch within a degree), on which two of the four branches of the
matrix -> quaternion conversion never run and every Jacobian block has only seen rotations about z.

Scenes: pgo_geometry_scenes.py (node rotations uniform on SO(3) with a table of special rotations on the first nodes, error rotations
up to 3 rad, sensor transforms with large rotations, odometry measurements on both sides of every OdomConvert threshold);
test_pgo_geometry_reference.py shows on the CPU that the reference alone meets what these tests rely on and that each check would catch
the fault it exists for.  Reference: np_reference on the oracle-flattened graph with the oracle's analytic Jacobians, as in
test_pgo_system_gpu.py, whose System / check_linearization / C_H (= 1e3, unchanged) these tests use.

Bounds (round-off, per entry):
  (a) node flattening: translations bit for bit; rotation entries C_H eps (matrix -> unit quaternion -> matrix);
  (b) xy-only flattening: z, the four structural zeros of Rz exactly 0, R[2][2] exactly 1; yaw within C_H eps / cos(pitch) of the oracle's
      (the condition number of atan2(2 (q0 q3 + q1 q2), 1 - 2 (q2^2 + q3^2)): both arguments carry the factor cos(pitch)), modulo 2 pi;
  (c) edge error norm: C_H eps s_k, s_k = 1 + |t_i| + |t_j| + |t_Z|;
  (d) H, b, chi2: check_linearization's.  Sensor variant: s_k gains the translation norms of the factors the measurement is composed
      from - both displacements, both sensor transforms and the raw `transform` (pgo_geometry_scenes.sensor_factor_magnitude).
      Derivation: Z = Df Sf T St^-1 Dt^-1 is four products, each of which rounds its translation at eps (|t_left| + |t_right|), so Z's
      translation is known to eps sum |t_factor| absolutely, however small |t_Z| itself comes out (here |t_T| reaches 10 m while the
      composed |t_Z| is that of the plain graph); System's s_k had only |t_Z|.  The odometry-threshold chain needs no such term,
      although the OdomConvert round trip passes through a turning radius of 3e6 m at theta = 1.001e-7: b sits at 1e-3 of the plain bound;
  (e), (g) trial poses: translations C_H eps (1 + |t| + |d_t|), rotation entries C_H eps;
  (f) the chi2 partials of the in-lane retraction and of the stored trial poses: bit for bit.

Measured on an MI355X, worst ratio to the bound (pytest -s prints the MEASURED table at the end of the module):
  (a) rotation entries after add_graph / set_graph                  4.0e-3 / 4.0e-3   (4 eps)
  (b) xy-only yaw                                                   3.3e-3
  (c) edge error norm, large-error graph                            1.1e-3
  (d) H / b / chi2    gentle 300/1200          initial              1.5e-4 / 2.7e-6 / 3.5e-9
                                               after optimize(5)    5.6e-4 / 2.7e-6 / 1.8e-11
                      large-error 300/1200     initial              1.4e-4 / 4.6e-6 / 6.3e-7
                      sensors 120/400          initial              1.2e-4 / 2.5e-6 / 2.1e-9
                                               after optimize(5)    3.1e-4 / 2.7e-6 / 6.7e-11
                      xy-only 300/1200         initial              1.0e-4 / 1.6e-5 / 1.1e-6
                                               after optimize(5)    4.5e-5 / 1.2e-5 / 0
                      odometry thresholds      initial              6.6e-5 / 1.0e-3 / 6.0e-7
  (e) trial translation / rotation, tumbling graph                  5.7e-4 / 6.0e-3;  after optimize(3) 6.8e-4 / 6.0e-3
  (g) trial translation / rotation, retraction edges                6.7e-4 / 3.0e-3
  (f) partials of the two chi2 launches: identical on every graph.  No ratio above 1: no device bug found at these edges.
"""
import numpy as np
import pytest

import np_reference as NP
import pgo_geometry_scenes as S
from test_pgo_system_gpu import C_H, System, _linearize_case, _note, _report, check_linearization  # noqa: F401  (_report: the MEASURED table)
from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _ratio(err, bound):
    r = np.asarray(err, np.float64) / np.asarray(bound, np.float64)
    return np.inf if not np.isfinite(r).all() else float(r.max())


def _diag(capi, g, sensors=None, **cfg):
    p = capi.DiagPgo(**cfg)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], sensors=sensors)
    return p


# ------------------------------------------------------------------------------------------------------------------ (a) node flattening
def _check_flattening(poses_in, poses_out, key):
    A = np.asarray(poses_in).reshape(-1, 3, 4); B = np.asarray(poses_out).reshape(-1, 3, 4)
    assert np.array_equal(A[:, :, 3], B[:, :, 3]), "translations changed on their way through the handle"
    w = _ratio(np.abs(A[:, :, :3] - B[:, :, :3]), C_H * EPS)
    _note("geometry: %s rotation entries / C_H eps" % key, w)
    assert w <= 1.0, "rotation entries differ from the input by %.3g x C_H eps at node %d" % (
        w, int(np.argmax(np.nan_to_num(np.abs(A[:, :, :3] - B[:, :, :3]), nan=np.inf).reshape(len(A), -1).max(1))))


def test_node_flattening_every_conversion_branch(capi, oracle):
    """store() right after add_graph (prepare_nodes_kernel) and after set_graph (prepare_flat_nodes_kernel), no optimize: 300 nodes (past
    one 256-lane workgroup), rotations from every branch of quat_from_R with the special table on the first nodes."""
    g = S.large_300()
    n = len(g["nodes_fixed"])
    br = S.conversion_branches(g["nodes_pose"].reshape(-1, 3, 4)[:, :, :3])
    assert min(br.values()) >= 50 and n > 256, br
    p = capi.Pgo()
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        _check_flattening(g["nodes_pose"], p.store()[0], "add_graph")
        fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        p.set_graph(fl["poses"], fl["fixed"], fl["ij"], fl["meas"], fl["info"], fl["robust"])
        _check_flattening(g["nodes_pose"], p.store()[0], "set_graph")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ (b) xy-only
def test_xy_only_flattening_with_real_roll_and_pitch(capi, oracle):
    g = S.xy_300()
    Rin = g["nodes_pose"].reshape(-1, 3, 4)[:, :, :3]
    cosp = np.hypot(Rin[:, 0, 0], Rin[:, 1, 0])                     # cos(pitch) of Rz Ry Rx
    assert cosp.min() >= np.cos(np.deg2rad(80.0)) * (1 - 1e-9) and cosp.min() <= 0.2
    p = _diag(capi, g, optimize_xy_only=1)
    try:
        P = p.linearize()["poses"].reshape(-1, 3, 4)
    finally:
        p.close()
    assert np.all(P[:, 2, 3] == 0.0)
    assert np.all(P[:, 0, 2] == 0.0) and np.all(P[:, 1, 2] == 0.0) and np.all(P[:, 2, 0] == 0.0) and np.all(P[:, 2, 1] == 0.0)
    assert np.all(P[:, 2, 2] == 1.0)
    assert np.array_equal(P[:, :2, 3], g["nodes_pose"].reshape(-1, 3, 4)[:, :2, 3])
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], optimize_xy_only=True)
    Q = fl["poses"].reshape(-1, 3, 4)
    yaw = np.arctan2(P[:, 1, 0], P[:, 0, 0]); yaw_ref = np.arctan2(Q[:, 1, 0], Q[:, 0, 0])
    d = np.abs(np.angle(np.exp(1j * (yaw - yaw_ref))))
    w = _ratio(d, C_H * EPS / cosp)
    _note("geometry: xy-only yaw / (C_H eps / cos pitch)", w)
    assert w <= 1.0, w
    assert np.abs(np.abs(yaw_ref[1:3]) - np.pi).max() <= 4 * EPS        # the scene: yaw = +pi, -pi ...
    assert np.array_equal(Rin[3], np.diag([1.0, -1, -1]))               # ... and roll = 180 degrees


# ------------------------------------------------------------------------------------------------------------------ (c) edge error
def test_edge_error_norms_at_large_error_rotations(capi, oracle):
    """store()'s per-edge |e| before any optimize (edge_error_kernel: edge_geom_of with the w < 0 flip, measurements from
    prepare_edges_kernel) on the large-error graph: error rotations of 1e-9 .. 3 rad, a zero-error edge, both signs of the raw w."""
    g = S.large_300()
    p = _diag(capi, g)
    try:
        poses, err, used = p.store()
        lin = p.linearize()
    finally:
        p.close()
    assert np.array_equal(poses, lin["poses"])
    R = System(oracle, g, lin)
    src = R.fl["src_edge"]
    assert np.array_equal(np.nonzero(used)[0], np.sort(src)) and np.isnan(err[used == 0]).all()
    want = np.linalg.norm(R.e, axis=1)
    w = _ratio(np.abs(err[src] - want), C_H * EPS * R.s)
    _note("geometry: edge error norm / C_H eps s_k (large-error graph)", w)
    assert w <= 1.0, w
    wq = S.raw_error_w(lin["poses"], R.fl["ij"], R.fl["meas"])
    assert (wq < 0).mean() >= 0.25 and (wq > 0).mean() >= 0.25 and np.abs(wq).min() >= 1e-3
    assert want.min() <= 1e-12 and want.max() >= 0.99                # the exact edge, and |q| = sin 1.5 at 3 rad


# ------------------------------------------------------------------------------------------------------------------ (d) linearisation
def test_linearization_gentle_tumbling_graph(capi, oracle):
    lin = _linearize_case(capi, oracle, S.gentle_300(), "geometry: gentle 300/1200", after=5)
    assert lin["row_ptr"][42] - lin["row_ptr"][0] > 256             # a workgroup's 42 rows span more than one 256-slot chunk


def test_linearization_large_error_graph(capi, oracle):
    g = S.large_300()
    lin = _linearize_case(capi, oracle, g, "geometry: large-error 300/1200")
    R = System(oracle, g, lin)
    chi = np.einsum("ki,kij,kj->k", R.e, R.fl["info"].reshape(-1, 6, 6), R.e)
    rb = R.fl["robust"] != 0
    assert (chi[rb] > 1.0).sum() >= 20 and (chi[rb] <= 1.0).sum() >= 20 and (~rb).sum() >= 20


def test_linearization_sensor_transforms_with_large_rotations(capi, oracle):
    g, sensors = S.sensor_variant(S.gentle_120(), seed=7)
    e = g["edges"]
    assert {-1, len(sensors)} <= set(e["sensor_from"].tolist()) and {-1, len(sensors)} <= set(e["sensor_to"].tolist())
    _linearize_case(capi, oracle, g, "geometry: sensors 120/400", sensors=sensors, after=5, extra=S.sensor_factor_magnitude(g, sensors))


def test_linearization_xy_only_tumbling_graph(capi, oracle):
    _linearize_case(capi, oracle, S.xy_300(), "geometry: xy-only 300/1200", cfg=dict(optimize_xy_only=1), after=5)


def test_linearization_odometry_threshold_chain(capi, oracle):
    g, cases = S.odometry_threshold_cases()
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], use_odometry_parameters=True)
    fl0 = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    assert np.abs(fl["meas"] - fl0["meas"]).max() > 1e-2             # the round trip does something
    _linearize_case(capi, oracle, g, "geometry: odometry thresholds", cfg=dict(use_odometry_parameters=1))


# ------------------------------------------------------------------------------------------------------------------ (e) (f) (g) trial
def _check_trial(p, dx, key, labels=None):
    """trial(dx) against se3_mul(X, fromVectorMQT(d)) at the poses the handle holds; the partials of the two chi2 launches bit for bit;
    fixed vertices untouched; the handle's current poses unchanged."""
    before = p.store()[0]
    lin = p.linearize()
    X = lin["poses"].reshape(-1, 3, 4)
    assert np.array_equal(before, lin["poses"])
    out = p.trial(dx, lam=0.5)
    assert np.array_equal(p.store()[0], before), "trial() moved the current poses"
    T = out["poses"].reshape(-1, 3, 4)
    fixed = lin["v2b"] < 0
    assert fixed.any() and np.abs(dx[fixed]).min() > 0, "the case hands no nonzero row to a fixed vertex"
    assert np.array_equal(T[fixed], X[fixed]), "a fixed vertex moved"
    d = np.where(fixed[:, None], 0.0, dx)
    want = NP.se3_mul(X, NP.from_vector_mqt(d))
    st = 1.0 + np.abs(X[:, :, 3]).max(1) + np.abs(d[:, :3]).max(1)
    et = np.abs(T[:, :, 3] - want[:, :, 3]).max(1); er = np.abs(T[:, :, :3] - want[:, :, :3]).reshape(len(T), -1).max(1)
    wt = _ratio(et, C_H * EPS * st); wr = _ratio(er, C_H * EPS)
    _note("geometry: %s trial translation / bound" % key, wt)
    _note("geometry: %s trial rotation / bound" % key, wr)
    worst = int(np.argmax(np.nan_to_num(er, nan=np.inf)))
    assert wt <= 1.0 and wr <= 1.0, (wt, wr, labels[worst] if labels else worst)
    assert len(out["part_inlane"]) >= 1
    assert np.array_equal(out["part_inlane"], out["part_stored"]), "chi2 of poses retracted in the edge lane is not chi2 of the stored trial poses"
    assert out["chi2_inlane"] == out["chi2_stored"]
    # computeScale = sum dx (lam dx + b) over the free vertices, against the b the hook linearised
    rows = lin["v2b"][~fixed]
    terms = d[~fixed] * (0.5 * d[~fixed] + lin["b"][rows])
    assert abs(out["scale"] - terms.sum()) <= C_H * EPS * np.abs(terms).sum()
    return lin, out


def test_trial_poses_and_chi2_on_a_tumbling_graph(capi, oracle):
    g = S.gentle_300()
    rng = np.random.default_rng(17)
    n = len(g["nodes_fixed"])
    dx = np.concatenate([rng.normal(0, 0.3, (n, 3)), rng.normal(0, 0.2, (n, 3))], axis=1)
    assert ((dx[:, 3:] ** 2).sum(1) < 1).all()
    p = _diag(capi, g)
    try:
        lin, out = _check_trial(p, dx, "tumbling")
        assert len(out["part_inlane"]) > 1                            # more than one workgroup of edges
        fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        chi = NP.chi2(out["poses"], fl["ij"], fl["meas"], fl["info"], fl["robust"])
        assert abs(out["chi2_stored"] - chi) <= 1e-9 * chi
        p.optimize(3)                                                 # ... and once more at poses the solver left (quaternions, not inputs)
        _check_trial(p, dx, "tumbling after optimize(3)")
    finally:
        p.close()


def test_retraction_edges_through_the_trial_hook(capi):
    """d_q = 0, |d_q|^2 = 0.75, w2 = 0 exactly (a half turn), w2 = -2^-52 and -0.28 (identity rotation, translation still applied),
    d_q = 1e-200: one vertex per case and base rotation, base rotations from every conversion branch."""
    g, dx, labels = S.retraction_graph()
    p = _diag(capi, g)
    try:
        lin, out = _check_trial(p, dx, "retraction edges", labels)
    finally:
        p.close()
    X = lin["poses"].reshape(-1, 3, 4); T = out["poses"].reshape(-1, 3, 4)
    for v, lab in enumerate(labels):
        if lab.startswith("w2 = -"):
            assert np.array_equal(T[v, :, :3], X[v, :, :3]), lab      # the guard: the stored quaternion is the old one, bit for bit
            assert not np.array_equal(T[v, :, 3], X[v, :, 3]), lab    # ... and the translation moved
        if lab.startswith("w2 = 0"):
            assert np.abs(T[v, :, :3] - X[v, :, :3] @ np.diag([1.0, -1, -1])).max() <= C_H * EPS, lab


def test_trial_hook_leaves_the_handle_usable(capi):
    """optimize after trial() gives the bits of an optimize on a handle that never saw the hook."""
    g = S.gentle_120()
    n = len(g["nodes_fixed"])
    dx = np.random.default_rng(3).normal(0, 0.2, (n, 6))
    res = []
    for hook in (False, True):
        p = _diag(capi, g)
        try:
            if hook:
                p.trial(dx, lam=0.5); p.trial(-dx)
            st = p.optimize(10)
            res.append((p.store()[0], st["chi2_final"], st["lm_trials"]))
        finally:
            p.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1:] == res[1][1:]


# ------------------------------------------------------------------------------------------------------------------ (h) end to end
@pytest.mark.parametrize("scene", ["gentle_120", "gentle_300"])
def test_end_to_end_against_the_oracle(capi, oracle, scene):
    from test_pgo_gpu import _check
    p = capi.Pgo()
    try:
        st, so = _check(p, oracle, getattr(S, scene)())
        assert st["chi2_final"] < st["chi2_initial"]
    finally:
        p.close()


def test_both_lm_loops_are_bit_identical_on_a_tumbling_graph(capi):
    from test_lm_loops_gpu import _same
    st = _same(capi, S.gentle_120())
    assert st["iterations_done"] >= 1


def test_batch_of_tumbling_graphs_equals_single_solves(capi, oracle):
    from test_batch_gpu import _single
    its = 20
    graphs = S.batch_120()
    bt = capi.PgoBatch(len(graphs))
    try:
        for k, g in enumerate(graphs):
            bt.graphs[k].add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        stats = bt.optimize(its)
        assert bt.n_batched == len(graphs)
        for k, g in enumerate(graphs):
            st1, poses1, err1 = _single(capi, g, its)
            poses, err, _ = bt.graphs[k].store()
            assert np.array_equal(poses, poses1), k
            assert np.array_equal(err, err1, equal_nan=True)
            for f in ("iterations_done", "lm_trials", "pcg_iterations", "precond_builds", "terminated_early", "n_edges", "n_gauge_fixed"):
                assert stats[k][f] == st1[f], (k, f, stats[k][f], st1[f])
            assert stats[k]["chi2_initial"] == st1["chi2_initial"] and stats[k]["chi2_final"] == st1["chi2_final"] and stats[k]["lambda_final"] == st1["lambda_final"]
        g = graphs[1]
        fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
        P, _ = oracle.pgo_optimize(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], iterations=its)
        dt, dr = synth.pose_errors(bt.graphs[1].store()[0].reshape(-1, 3, 4), P.reshape(-1, 3, 4))
        assert dt < 1e-3 and dr < 1e-4, (dt, dr)
    finally:
        bt.close()
