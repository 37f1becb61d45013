"""Scenes for the geometry of the pose-graph solve (test_pgo_geometry_reference.py on the CPU, test_pgo_geometry_gpu.py on the device):
rotations all over SO(3) and at the edges of every branch of the matrix -> quaternion conversion, error rotations up to 3 rad, sensor
transforms with large rotations, and odometry measurements on both sides of every threshold of the OdomConvert round trip.  Plain NumPy.

synth.make_pose_graph - the only generator the device tests had - draws a planar trajectory whose roll and pitch stay within a degree:
two of the four conversion branches, the w < 0 flip at large angles, the non-z Jacobian blocks and the odometry thresholds never ran.
"""
import numpy as np

from uzliti_slam_amd import synth

ODOM_THRESHOLD = 1e-7             # every threshold of OdomConvert (oracle/uzl_oracle_pgo.c: uzlo_odom_convert)
ERROR_ANGLES = (1e-9, 0.05, 0.5, 1.5, 2.5, 3.0)      # rad; 3.0 at most: the unit error quaternion keeps |w| >= cos 1.5 = 0.07


# ------------------------------------------------------------------------------------------------------------------ rotations
def rot(axis, angle):
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def half_turn(axis):
    """180 degrees about `axis`, R = 2 n n^T - I with n n^T formed from the INTEGER axis: the entries that tie are equal to the bit."""
    a = np.asarray(axis, np.float64)
    return 2.0 * np.outer(a, a) / float(a @ a) - np.eye(3)


def random_rotations(rng, k):
    """Uniform on SO(3): normalised Gaussian quaternions."""
    q = rng.normal(size=(k, 4))
    return synth.quat_to_R(q / np.linalg.norm(q, axis=1, keepdims=True))


def euler_R(roll, pitch, yaw):
    """fromEuler (isometry3d_mappings.cpp:59-75): Rz(yaw) Ry(pitch) Rx(roll)."""
    roll, pitch, yaw = (np.asarray(v, np.float64) for v in (roll, pitch, yaw))
    sy, cy = np.sin(yaw * 0.5), np.cos(yaw * 0.5)
    sp, cp = np.sin(pitch * 0.5), np.cos(pitch * 0.5)
    sr, cr = np.sin(roll * 0.5), np.cos(roll * 0.5)
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)
    return synth.quat_to_R(q)


def special_rotations():
    """(name, R) at the edges of Eigen's Quaterniond(Matrix3d): trace = 0, trace = -1 with two and three equal diagonal entries, angles
    next to pi and next to 0."""
    d111 = np.array([1.0, 1.0, 1.0])
    third = 2 * np.pi / 3
    gen = np.array([0.3, -0.5, 0.81])
    return [
        ("identity", np.eye(3)),
        ("180 x", half_turn([1, 0, 0])), ("180 y", half_turn([0, 1, 0])), ("180 z", half_turn([0, 0, 1])),
        ("180 (1,1,0)", half_turn([1, 1, 0])), ("180 (1,0,1)", half_turn([1, 0, 1])), ("180 (0,1,1)", half_turn([0, 1, 1])),
        ("180 (1,1,1)", half_turn([1, 1, 1])),
        ("120 (1,1,1) cyclic permutation", np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])),
        ("120 - 1e-9 (1,1,1)", rot(d111, third - 1e-9)), ("120 + 1e-9 (1,1,1)", rot(d111, third + 1e-9)),
        ("pi - 1e-5 x", rot([1, 0, 0], np.pi - 1e-5)), ("pi - 1e-5 y", rot([0, 1, 0], np.pi - 1e-5)),
        ("pi - 1e-9 general axis", rot(gen, np.pi - 1e-9)),
        ("+90 x", rot([1, 0, 0], np.pi / 2)), ("-90 x", rot([1, 0, 0], -np.pi / 2)),
        ("+90 y", rot([0, 1, 0], np.pi / 2)), ("-90 y", rot([0, 1, 0], -np.pi / 2)),
        ("1e-9 rad", rot(gen, 1e-9)),
    ]


def conversion_branch(R):
    """The branch Eigen's rule gives a matrix: 'w' when trace > 0, else i = 0 unless m11 > m00, then i = 2 if m22 > m_ii."""
    m = np.asarray(R, np.float64).reshape(3, 3)
    if m[0, 0] + m[1, 1] + m[2, 2] > 0.0:
        return "w"
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    return i


def conversion_branches(Rs):
    Rs = np.asarray(Rs, np.float64).reshape(-1, 3, 3)
    out = {"w": 0, 0: 0, 1: 0, 2: 0}
    for R in Rs:
        out[conversion_branch(R)] += 1
    return out


def quat_from_R_branch(R, branch=None, swap12=False):
    """Quaterniond(Matrix3d) (w, x, y, z) through the branch given (None: the rule's), one rounding per operation as the C oracle
    (compiled without contraction).  swap12: the fault of the sensitivity dry run - the conditions of i = 1 and i = 2 exchanged."""
    m = np.asarray(R, np.float64).reshape(3, 3)
    if branch is None:
        branch = conversion_branch(m)
        if swap12 and branch in (1, 2):
            branch = 3 - branch
    q = np.empty(4)
    if branch == "w":
        t = np.sqrt((m[0, 0] + m[1, 1] + m[2, 2]) + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2, 1] - m[1, 2]) * t; q[2] = (m[0, 2] - m[2, 0]) * t; q[3] = (m[1, 0] - m[0, 1]) * t
        return q
    i = int(branch); j = (i + 1) % 3; k = (j + 1) % 3
    t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + 1.0)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (m[k, j] - m[j, k]) * t
    q[1 + j] = (m[j, i] + m[i, j]) * t
    q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def unit_quats(Rs, **kw):
    q = np.array([quat_from_R_branch(R, **kw) for R in np.asarray(Rs, np.float64).reshape(-1, 3, 3)])
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def raw_error_w(poses, ij, meas):
    """w of the error quaternion BEFORE the flip to w >= 0, as the solver forms it: q_a (x) (conj(q_i) (x) q_j) with q_a = conj(q(Z)) and
    every q the normalised conversion of its matrix, sign as the conversion leaves it (csrc/pgo_kernels.hip: edge_geom_of)."""
    X = np.asarray(poses, np.float64).reshape(-1, 3, 4); Z = np.asarray(meas, np.float64).reshape(-1, 3, 4)
    ij = np.asarray(ij).reshape(-1, 2)
    conj = np.array([1.0, -1, -1, -1])
    qx = unit_quats(X[:, :, :3]); qz = unit_quats(Z[:, :, :3])
    qb = synth.quat_mul(qx[ij[:, 0]] * conj, qx[ij[:, 1]])
    return synth.quat_mul(qz * conj, qb)[:, 0]


# ------------------------------------------------------------------------------------------------------------------ graphs
def _info(rng, n_chain, n_loop):
    """Information matrices on synth.make_pose_graph's scale."""
    odom_info = np.zeros((6, 6))
    odom_info[:3, :3] = np.eye(3) / (0.02 ** 2)
    odom_info[3:, 3:] = np.eye(3) / (0.02 ** 2 * 0.05 ** 2)
    c = rng.uniform(20, 300, n_loop); m = rng.uniform(0.02, 0.08, n_loop)
    s = 0.1 * c / m
    linfo = np.zeros((n_loop, 6, 6))
    for k in range(3):
        linfo[:, k, k] = s; linfo[:, 3 + k, 3 + k] = 100.0 * s
    return np.concatenate([np.tile(odom_info.reshape(1, 36), (n_chain, 1)), linfo.reshape(-1, 36)])


def _edge_dict(frm, to, types, Z, info, diff_time):
    E = len(frm)
    I12 = np.tile(np.eye(3, 4).reshape(1, 12), (E, 1))
    return {"from": np.asarray(frm, np.int32), "to": np.asarray(to, np.int32), "type": np.asarray(types, np.int32),
            "sensor_from": np.full(E, -1, np.int32), "sensor_to": np.full(E, -1, np.int32), "valid": np.ones(E, np.int32),
            "transform": np.asarray(Z, np.float64).reshape(E, 12), "displacement_from": I12.copy(), "displacement_to": I12.copy(),
            "information": np.asarray(info, np.float64).reshape(E, 36), "diff_time": np.asarray(diff_time, np.float64)}


def _rand_axes(rng, k):
    a = rng.normal(size=(k, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def tumbling_graph(n, e, seed, variant="gentle", outlier_frac=0.05, max_pitch_deg=None, sig_init=(0.05, 0.02)):
    """A pose graph in synth.make_pose_graph's layout whose node rotations are uniform on SO(3), the special table on the first nodes
    (node 0, the fixed one, is the identity); positions uniform in a 10 m box; a chain typed as odometry (not robust) plus random
    TYPE_3D_FULL edges (robust), either direction; measurement = true relative pose x noise.

    variant "gentle": for end-to-end solves.  Noise as synth's (odometry 2 cm / 1 mrad, features 5 cm / 10 mrad), a share `outlier_frac`
        of the feature edges gross (+-2 m, +-0.5 rad per axis), initial poses = truth x a perturbation of sig_init (m, rad).
    variant "large": every edge's noise rotation has an angle drawn from ERROR_ANGLES about a random axis; its noise translation is 1 cm
        (1 mm on the odometry chain).  The initial ROTATIONS are the truth's, so the error rotation of an edge is its noise rotation
        (<= 3 rad) to rounding; half of the vertices start 0.2 m off in translation, which leaves edges between the others whose robust
        kernel is inactive.  The last edge's measurement is exactly the composed relative pose of its (unperturbed) ends.
    max_pitch_deg: node rotations from Euler angles instead, yaw and roll uniform, |pitch| below the limit, led by yaw = +pi, yaw = -pi,
        roll = 180 degrees and pitch = +-limit (for optimize_xy_only: the projection's yaw has condition number 1 / cos(pitch))."""
    rng = np.random.default_rng(seed)
    n = int(n); n_loop = int(e) - (n - 1)
    assert n_loop >= 1 and variant in ("gentle", "large")
    if max_pitch_deg is None:
        R = random_rotations(rng, n)
        table = [r for _, r in special_rotations()]
    else:
        lim = np.deg2rad(max_pitch_deg)
        R = euler_R(rng.uniform(-np.pi, np.pi, n), rng.uniform(-lim, lim, n), rng.uniform(-np.pi, np.pi, n))
        table = [np.eye(3), np.diag([-1.0, -1, 1]), euler_R(0.0, 0.0, -np.pi), np.diag([1.0, -1, -1]), euler_R(0.3, lim, 1.0),
                 euler_R(-2.0, -lim, -3.0), euler_R(np.pi, 0.5, np.pi)]
    R[:len(table)] = np.array(table)[:n]
    t = rng.uniform(-5.0, 5.0, (n, 3))
    gt = synth.se3(R, t)
    lf = rng.integers(0, n, n_loop); lt = (lf + rng.integers(1, n, n_loop)) % n          # never a self-loop
    frm = np.concatenate([np.arange(n - 1), lf]); to = np.concatenate([np.arange(1, n), lt])
    E = len(frm)
    odom = np.arange(E) < n - 1
    rel = synth.se3_mul(synth.se3_inv(gt[frm]), gt[to])
    if variant == "gentle":
        sig_t = np.where(odom, 0.02, 0.05)[:, None]; sig_r = np.where(odom, 0.001, 0.01)[:, None]
        noise = synth.se3_from_noise(rng.normal(size=(E, 3)) * sig_t, rng.normal(size=(E, 3)) * sig_r)
        outl = (rng.random(E) < outlier_frac) & ~odom
        gross = synth.se3_from_noise(rng.uniform(-2, 2, (E, 3)), rng.uniform(-0.5, 0.5, (E, 3)))
        noise = np.where(outl[:, None, None], gross, noise)
        init = gt.copy()
        init[1:] = synth.se3_mul(gt[1:], synth.se3_from_noise(rng.normal(0, sig_init[0], (n - 1, 3)), rng.normal(0, sig_init[1], (n - 1, 3))))
    else:
        ang = np.asarray(ERROR_ANGLES)[rng.integers(0, len(ERROR_ANGLES), E)]
        noise = synth.se3(np.array([rot(a, th) for a, th in zip(_rand_axes(rng, E), ang)]),
                          rng.normal(size=(E, 3)) * np.where(odom, 0.001, 0.01)[:, None])
        noise[-1] = np.eye(3, 4)
        outl = np.zeros(E, bool)
        off = rng.random(n) < 0.5
        off[0] = False; off[frm[-1]] = False; off[to[-1]] = False
        init = gt.copy()
        init[off, :, 3] += rng.normal(0, 0.2, (int(off.sum()), 3))
    Z = synth.se3_mul(rel, noise)
    types = np.where(odom, synth.EDGE_TYPE_ODOM, synth.EDGE_TYPE_3D_FULL)
    edges = _edge_dict(frm, to, types, Z, _info(rng, n - 1, n_loop), np.where(odom, 0.5, 0.0))
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    return dict(nodes_pose=init.reshape(n, 12), nodes_fixed=fixed, gt_pose=gt.reshape(n, 12), edges=edges, n_outliers=int(outl.sum()))


def sensor_variant(g, seed):
    """The same graph with a table of sensor transforms and per-edge displacements whose rotations are large (rotation vectors of scale
    1.5, entries of the special table among them), folded into `transform` as test_pgo_gpu.test_sensor_transforms_and_displacements does,
    so that the composed measurement is the one of `g`.  Sensor indices run from -1 to one past the end of the table (both: identity).
    Returns (graph, sensors [K,12])."""
    rng = np.random.default_rng(seed)
    g = dict(g); e = {k: np.array(v) for k, v in g["edges"].items()}
    E = len(e["from"])
    sp = dict(special_rotations())

    def rand_T(k, ts):
        return synth.se3(synth.quat_to_R(synth.quat_from_rotvec(rng.normal(0, 1.5, (k, 3)))), rng.normal(0, ts, (k, 3)))

    S = rand_T(6, 0.5)
    S[3, :, :3] = sp["180 x"]; S[4, :, :3] = sp["180 (1,1,0)"]; S[5, :, :3] = sp["120 (1,1,1) cyclic permutation"]
    K = len(S)
    sf = rng.integers(-1, K + 1, E).astype(np.int32); st = rng.integers(-1, K + 1, E).astype(np.int32)
    sf[:4] = [-1, K, 3, 5]; st[:4] = [K, -1, 5, 4]
    Df = rand_T(E, 0.5); Dt = rand_T(E, 0.5)
    Df[0, :, :3] = sp["180 (1,1,1)"]; Dt[1, :, :3] = sp["180 y"]
    I = np.eye(3, 4)[None]
    tab = np.concatenate([I, S, I])                                   # index -1 and index K: identity
    Sf = tab[sf + 1]; St = tab[st + 1]
    T = e["transform"].reshape(-1, 3, 4)
    odom = e["type"] == synth.EDGE_TYPE_ODOM
    # feature: Z = Df Sf T' St^-1 Dt^-1  =>  T' = Sf^-1 Df^-1 Z Dt St ; odometry: T' = Df^-1 Z Dt
    Tf = synth.se3_mul(synth.se3_mul(synth.se3_inv(Sf), synth.se3_inv(Df)), synth.se3_mul(synth.se3_mul(T, Dt), St))
    To = synth.se3_mul(synth.se3_inv(Df), synth.se3_mul(T, Dt))
    e["transform"] = np.where(odom[:, None, None], To, Tf).reshape(-1, 12)
    e["displacement_from"] = Df.reshape(-1, 12); e["displacement_to"] = Dt.reshape(-1, 12)
    e["sensor_from"] = sf; e["sensor_to"] = st
    g["edges"] = e
    return g, S.reshape(-1, 12)


def sensor_factor_magnitude(g, sensors):
    """Per input edge, the translation norms of the factors the composed measurement is built from besides `transform`: both
    displacements and both sensor transforms (max-norm of each translation, as System's s_k takes them)."""
    e = g["edges"]
    S = np.asarray(sensors, np.float64).reshape(-1, 3, 4)
    K = len(S)
    tab = np.concatenate([np.zeros(1), np.abs(S[:, :, 3]).max(1), np.zeros(1)])
    sf = np.clip(np.asarray(e["sensor_from"]), -1, K); st = np.clip(np.asarray(e["sensor_to"]), -1, K)
    Df = np.asarray(e["displacement_from"]).reshape(-1, 3, 4); Dt = np.asarray(e["displacement_to"]).reshape(-1, 3, 4)
    T = np.asarray(e["transform"]).reshape(-1, 3, 4)
    odom = np.asarray(e["type"]) == synth.EDGE_TYPE_ODOM
    return np.abs(Df[:, :, 3]).max(1) + np.abs(Dt[:, :, 3]).max(1) + np.abs(T[:, :, 3]).max(1) + np.where(odom, 0.0, tab[sf + 1] + tab[st + 1])


# ------------------------------------------------------------------------------------------------------------------ odometry thresholds
def odometry_threshold_cases(seed=3):
    """A chain whose odometry measurements put the OdomConvert round trip (use_odometry_parameters) on both sides of each of its
    thresholds: |theta| against 1e-7, |diff_time| against 1e-7, |vr - vl| against 1e-7.  Returns (graph, cases): cases is a list of
    dict(x, y, theta, dt, z, roll, pitch) - edge k of the graph carries case k.  Every case stays 1e-4 relative clear of a threshold."""
    rng = np.random.default_rng(seed)
    cases = []
    thetas = (0.0, 0.999e-7, -0.999e-7, 1.001e-7, -1.001e-7, 1e-3, 3.0)
    dts = (0.0, 0.999e-7, 1.001e-7, 0.5, -0.8)
    for th in thetas:
        for dt in dts:
            cases.append(dict(x=0.3, y=0.04, theta=th, dt=dt))                    # lateral slip, turning and straight
    for th, dt in ((2e-7, 1.9), (2e-7, 2.1), (-2e-7, 1.9), (-2e-7, -2.1), (1e-3, 9.9e3), (1e-3, 1.01e4)):
        cases.append(dict(x=0.3, y=0.0, theta=th, dt=dt))                         # |vr - vl| = |theta / dt| on both sides of 1e-7
    for R_, th, dt in ((2.0, 0.3, 0.5), (-1.5, 0.2, 1.0), (0.4, 1.2, 0.1)):       # exact arcs: the round trip is the identity
        cases.append(dict(x=R_ * np.sin(th), y=R_ * (1 - np.cos(th)), theta=th, dt=dt))
    cases.append(dict(x=0.3, y=0.0, theta=0.0, dt=0.5))                           # straight, no slip
    cases.append(dict(x=-0.3, y=0.1, theta=0.0, dt=0.5))                          # straight backwards with slip: hypot drops the sign
    cases.append(dict(x=0.3, y=0.1, theta=0.2, dt=1.0))                           # slip on a turning motion
    lim = np.deg2rad(80.0)
    for k, c in enumerate(cases):
        c["z"] = float(rng.uniform(-0.5, 0.5))
        c["roll"] = float(rng.uniform(-lim, lim)); c["pitch"] = float(rng.uniform(-lim, lim))
    cases[0].update(z=0.0, roll=0.0, pitch=0.0)
    cases[3].update(roll=lim * 0.999, pitch=-lim * 0.999)
    cases[28].update(roll=-lim * 0.999, pitch=lim * 0.999)
    m = len(cases)
    Z = np.stack([synth.se3(euler_R(c["roll"], c["pitch"], c["theta"]), np.array([c["x"], c["y"], c["z"]])) for c in cases])
    n = m + 1
    gt = np.empty((n, 3, 4)); gt[0] = np.eye(3, 4)
    for i in range(m):
        gt[i + 1] = synth.se3_mul(gt[i], Z[i])
    odom_info = np.zeros((6, 6))
    odom_info[:3, :3] = np.eye(3) / (0.02 ** 2)
    odom_info[3:, 3:] = np.eye(3) / (0.02 ** 2 * 0.05 ** 2)
    edges = _edge_dict(np.arange(m), np.arange(1, n), np.full(m, synth.EDGE_TYPE_ODOM), Z, np.tile(odom_info.reshape(1, 36), (m, 1)),
                       [c["dt"] for c in cases])
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    return dict(nodes_pose=gt.reshape(n, 12).copy(), nodes_fixed=fixed, gt_pose=gt.reshape(n, 12), edges=edges), cases


def odom_branch_inputs(theta, x, y, dt):
    """The quantities uzlo_odom_convert branches on, restated: (|theta|, |dt|, |vr - vl|)."""
    dt = abs(dt)
    if abs(theta) > ODOM_THRESHOLD:
        c, s = np.cos(theta), np.sin(theta)
        y2 = 10.0
        x4 = (c * 0.0 - s * y2) + x; y4 = (s * 0.0 + c * y2) + y
        R = (y2 * (x * y4 - y * x4)) / (y2 * (x - x4))
        w = theta / dt if dt > ODOM_THRESHOLD else 0.0
        vl = (2.0 * R * w - w) / 2.0
        vr = w + vl
    else:
        vl = vr = np.hypot(x, y) / dt if dt > ODOM_THRESHOLD else 0.0
    return abs(theta), dt, abs(vr - vl)


# ------------------------------------------------------------------------------------------------------------------ retraction
def retraction_cases():
    """(name, d_q) of test (g): both sides of w2 = 1 - |d_q|^2 = 0 and its ends."""
    return [("d_q = 0", (0.0, 0.0, 0.0)), ("|d_q|^2 = 0.75", (0.5, 0.5, 0.5)), ("w2 = 0: half turn", (1.0, 0.0, 0.0)),
            ("w2 = -2^-52", (1.0, 2.0 ** -26, 0.0)), ("w2 = -0.28", (0.8, 0.8, 0.0)), ("d_q = 1e-200", (1e-200, 0.0, 0.0))]


def retraction_graph(seed=5):
    """One free vertex per (retraction case x base rotation), base rotations from every conversion branch and the ties; vertex 0 fixed,
    a chain plus a few closures.  Returns (graph, dx [n,6], labels): dx carries the case's d_q and a translation of a metre or so;
    row 0 (the fixed vertex) is nonzero on purpose."""
    rng = np.random.default_rng(seed)
    sp = dict(special_rotations())
    bases = [sp["identity"], sp["180 x"], sp["180 y"], sp["180 z"], sp["180 (1,1,0)"], sp["180 (1,1,1)"],
             sp["120 (1,1,1) cyclic permutation"], sp["pi - 1e-9 general axis"]] + list(random_rotations(rng, 8))
    cases = retraction_cases()
    R = [np.eye(3)]; dq = [(0.3, -0.2, 0.1)]; labels = ["fixed"]
    for name, d in cases:
        for b, B in enumerate(bases):
            R.append(B); dq.append(d); labels.append("%s / base %d" % (name, b))
    n = len(R)
    gt = synth.se3(np.array(R), rng.uniform(-5, 5, (n, 3)))
    n_loop = 40
    lf = rng.integers(0, n, n_loop); lt = (lf + rng.integers(1, n, n_loop)) % n
    frm = np.concatenate([np.arange(n - 1), lf]); to = np.concatenate([np.arange(1, n), lt])
    E = len(frm)
    odom = np.arange(E) < n - 1
    Z = synth.se3_mul(synth.se3_mul(synth.se3_inv(gt[frm]), gt[to]), synth.se3_from_noise(rng.normal(0, 0.05, (E, 3)), rng.normal(0, 0.01, (E, 3))))
    edges = _edge_dict(frm, to, np.where(odom, synth.EDGE_TYPE_ODOM, synth.EDGE_TYPE_3D_FULL), Z, _info(rng, n - 1, n_loop), np.where(odom, 0.5, 0.0))
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    dx = np.concatenate([rng.normal(0, 1.0, (n, 3)), np.array(dq)], axis=1)
    return dict(nodes_pose=gt.reshape(n, 12).copy(), nodes_fixed=fixed, gt_pose=gt.reshape(n, 12), edges=edges), dx, labels


# ------------------------------------------------------------------------------------------------------------------ the committed scenes
def gentle_120():
    return tumbling_graph(120, 400, seed=101)


def gentle_300():
    return tumbling_graph(300, 1200, seed=102)


def large_300():
    return tumbling_graph(300, 1200, seed=103, variant="large")


def xy_300():
    """(no rotation in the initial perturbation: the input rotations are the table's and keep the pitch limit)"""
    return tumbling_graph(300, 1200, seed=104, max_pitch_deg=80.0, sig_init=(0.05, 0.0))


def batch_120():
    return [tumbling_graph(120, 400, seed=201 + k) for k in range(3)]
