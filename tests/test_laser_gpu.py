"""GPU tests of uzl_laser_* (laser scan matching): the stage entry equals the NumPy restatement tests/laser_reference.py exactly
(steps 1-4: host table, f64, no FMA); the whole solve equals it in every integer and within the project's pose bound; a pair's
result does not depend on the batch; the handle's edges; depth images -> laser line -> laser store on the device equals the
round trip through the host; and a returned edge closes a loop in the pose-graph solver."""
import math

import numpy as np
import pytest

import laser_reference as LR
import laser_scenes as LS
import laserline_scenes as LLS

pytestmark = pytest.mark.gpu

SCENES = LS.scenes()
NAMES = list(SCENES)
CASES = [(n, g) for n in NAMES for g in range(len(LS.GUESSES))]
# Largest relative difference of `information` (max |device - restatement| / max |restatement| over the 6x6) measured on CASES at
# the first GPU run: see INFO_REL_MEASURED in DESIGN.md, "Laser scan matching".  Asserted at ten times that.
INFO_REL_MEASURED = 4.131e-16
_shared = {}


def guess(name, g):
    return LS.displaced(SCENES[name]["true"], *LS.GUESSES[g])


@pytest.fixture(scope="module")
def store(capi):
    """one handle with every scene's scans (scan 2 k = from, 2 k + 1 = to of scene k) and the restatement's results, computed once"""
    h = capi.Laser()
    scans = []
    for n in NAMES:
        scans += [SCENES[n]["scan_from"], SCENES[n]["scan_to"]]
    assert h.add_scans(scans) == 0 and h.scan_count() == 2 * len(NAMES)
    if "want" not in _shared:
        _shared["want"] = {(n, g): LR.estimate(SCENES[n]["scan_from"], SCENES[n]["scan_to"], guess(n, g)) for n, g in CASES}
    yield h, _shared["want"]
    h.close()


def pair(name, g):
    k = NAMES.index(name)
    return (2 * k, 2 * k + 1, guess(name, g))


@pytest.mark.parametrize("name", ["room8", "closet37", "room", "room_invalid"])
def test_stage_equals_the_restatement_exactly(capi, store, name):
    h, _ = store
    s = SCENES[name]
    k = NAMES.index(name)
    F, T = LR.points(s["scan_from"]), LR.points(s["scan_to"])
    seen = 0
    for g in range(len(LS.GUESSES)):
        G = guess(name, g)
        th = math.atan2(G[1, 0], G[0, 0])
        got = h.correspondences(2 * k, 2 * k + 1, (G[0, 3], G[1, 3], th), s["n"])
        want = LR.correspondences(F, T, (G[0, 3], G[1, 3], math.cos(th), math.sin(th)), LR.DEFAULTS)
        for a, b, what in zip(got, want, ("j1", "j2", "valid", "dist")):
            assert a.dtype == b.dtype
            assert np.array_equal(a.view(np.uint64) if what == "dist" else a, b.view(np.uint64) if what == "dist" else b), \
                (what, g, np.flatnonzero(a != b)[:8].tolist())
        seen += int(want[2].sum())
    if s["n"] >= 37:
        assert seen > 0


def test_stage_at_the_true_pose_of_the_eight_beam_scan(capi, store):
    """the 8-beam scene has correspondences only near its true pose (beams 45 degrees apart)"""
    h, _ = store
    s = SCENES["room8"]
    k = NAMES.index("room8")
    cfg = LR.config(max_correspondence_dist=0.3)
    x = s["true"]
    got = h.correspondences(2 * k, 2 * k + 1, x, 8)
    want = LR.correspondences(s["scan_from"], s["scan_to"], (x[0], x[1], math.cos(x[2]), math.sin(x[2])), cfg)
    assert want[2].sum() >= 4
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


def test_the_largest_scan(capi):
    """4096 beams, the most a scan may have (16 strips per lane, 144 KiB of LDS): the stage equals the restatement exactly and the
    solve recovers the true pose within the restatement's bound (tests/test_laser_reference.py)"""
    a, b = (2.0, 1.5, 0.1), (2.6, 1.9, 0.45)
    s = LS.make("room4096", LS.ROOM, a, b, 4096, -math.pi, 2 * math.pi / 4096)
    h = capi.Laser()
    assert h.add_scans([s["scan_from"], s["scan_to"]]) == 0
    G = LS.displaced(s["true"], *LS.GUESSES[1])
    th = math.atan2(G[1, 0], G[0, 0])
    got = h.correspondences(0, 1, (G[0, 3], G[1, 3], th), 4096)
    want = LR.correspondences(s["scan_from"], s["scan_to"], (G[0, 3], G[1, 3], math.cos(th), math.sin(th)), LR.DEFAULTS)
    for x, y, what in zip(got, want, ("j1", "j2", "valid", "dist")):
        assert x.tobytes() == y.tobytes(), (what, np.flatnonzero(x != y)[:8].tolist())
    assert want[2].sum() > 1000
    e = h.estimate([(0, 1, G), (1, 0, np.eye(3, 4))])
    h.close()
    T = e[0]["transform"].reshape(3, 4)
    dt = math.hypot(T[0, 3] - s["true"][0], T[1, 3] - s["true"][1])
    dr = abs(math.atan2(math.sin(math.atan2(T[1, 0], T[0, 0]) - s["true"][2]), math.cos(math.atan2(T[1, 0], T[0, 0]) - s["true"][2])))
    print("4096 beams: status %d it %d nvalid %d of %d: %.3e m %.3e rad" % (e[0]["status"], e[0]["iterations"], e[0]["nvalid"], e[0]["scan_valid"], dt, dr))
    assert e[0]["status"] == capi.LASER_OK and e[0]["scan_valid"] == 4096 and e[0]["nvalid"] > 1000
    assert dt < 2 * 2.62e-4 and dr < 2 * 3.15e-4


def info_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_solve_equals_the_restatement(capi, store):
    h, want = store
    got = h.estimate([pair(n, g) for n, g in CASES])
    worst = 0.0
    for (n, g), e in zip(CASES, got):
        w = want[(n, g)]
        line = (n, g, int(e["status"]), int(e["iterations"]), int(e["nvalid"]), int(e["scan_valid"]), int(e["deg_count"]))
        assert line[2:] == (w["status"], w["iterations"], w["nvalid"], w["scan_valid"], w["deg_count"]), (line, w)
        assert e["matching_score"] == w["matching_score"]
        if w["status"] in (LR.FEW_CORR, LR.DEGENERATE) and w["iterations"] == 0:
            assert np.array_equal(e["transform"].reshape(3, 4), w["transform"])
            continue
        T = e["transform"].reshape(3, 4)
        dt = math.hypot(T[0, 3] - w["x"][0], T[1, 3] - w["x"][1])
        dr = abs(math.atan2(T[1, 0] * w["x"][2] - T[0, 0] * w["x"][3], T[0, 0] * w["x"][2] + T[1, 0] * w["x"][3]))
        rel = info_rel(e["information"].reshape(6, 6), w["information"])
        print("%-13s guess %d status %d it %d nvalid %d: dt %.3e m dr %.3e rad information rel %.3e error %.6e / %.6e"
              % (n, g, line[2], line[3], line[4], dt, dr, rel, e["error"], w["error"]))
        if w["status"] == LR.OK:                                  # README "Parity": 1e-3 m / 1e-4 rad
            assert dt < 1e-3 and dr < 1e-4
            assert T[2].tolist() == [0, 0, 1, 0] and T[0, 2] == 0 and T[1, 2] == 0 and T[0, 1] == -T[1, 0] and T[0, 0] == T[1, 1]
            assert abs(e["error"] - w["error"]) <= 1e-6 * w["error"] + 1e-10
            worst = max(worst, rel)
    print("largest relative difference of information: %.3e" % worst)
    assert worst <= 10 * INFO_REL_MEASURED
    assert sum(1 for n, g in CASES if want[(n, g)]["status"] == LR.OK) >= 12


def mixed_pairs():
    out = [pair(n, g) for n, g in CASES] + [pair(n, g) for n, g in CASES]
    k = NAMES.index
    out += [(2 * k("room"), 2 * k("room_invalid") + 1, guess("room", 1)), (2 * k("room") + 1, 2 * k("room") + 1, np.eye(3, 4)),
            (2 * k("closet37"), 2 * k("room8"), np.eye(3, 4))]
    return out[:33]


def test_batch_independence(capi, store):
    """33 pairs mixing all scenes (beam counts 8, 37 and 720 in one launch) = 33 calls of one pair each, bit for bit; and reversed"""
    h, _ = store
    pairs = mixed_pairs()
    assert len(pairs) == 33
    batch = h.estimate(pairs)
    single = np.concatenate([h.estimate([p]) for p in pairs])
    assert batch.tobytes() == single.tobytes()
    rev = h.estimate(pairs[::-1])
    assert rev[::-1].tobytes() == batch.tobytes()
    assert len(set(int(s) for s in batch["status"])) >= 2


def test_edges_of_the_handle(capi, store):
    h, _ = store
    room, corridor = NAMES.index("room"), NAMES.index("corridor")
    n0 = h.scan_count()
    empty = h.add_scans([LS.empty_scan()])
    assert empty == n0
    e = h.estimate([(2 * room, empty, np.eye(3, 4))])[0]
    assert e["status"] == capi.LASER_FEW_CORR and e["scan_valid"] == 0 and e["matching_score"] == 0
    # identical scans, identity guess
    e = h.estimate([(2 * room, 2 * room, np.eye(3, 4))])[0]
    T = e["transform"].reshape(3, 4)
    assert e["status"] == capi.LASER_OK and e["iterations"] == 1 and e["nvalid"] == e["scan_valid"] == 720
    assert abs(T[0, 3]) < 1e-12 and abs(T[1, 3]) < 1e-12 and abs(math.atan2(T[1, 0], T[0, 0])) < 1e-12
    # 3 m away
    c = SCENES["corridor"]
    e = h.estimate([(2 * corridor, 2 * corridor + 1, LS.displaced(c["true"], 3.0, 0.0, 0.0))])[0]
    assert e["status"] == capi.LASER_FEW_CORR and e["iterations"] == 0
    # converges, but moves further than the limits allow
    tight = capi.Laser(max_linear_correction=0.3)
    tight.add_scans([SCENES["room"]["scan_from"], SCENES["room"]["scan_to"]])
    e = tight.estimate([(0, 1, guess("room", 0))])[0]
    ok = h.estimate([pair("room", 0)])[0]
    assert e["status"] == capi.LASER_TOO_FAR and e["matching_score"] == 0 and e["nvalid"] == ok["nvalid"] > 0
    assert ok["status"] == capi.LASER_OK and np.array_equal(e["transform"], ok["transform"])
    tight.close()
    # nothing to do, and bad arguments change nothing
    assert len(h.estimate([])) == 0
    before = h.estimate([pair("room", 1)]).tobytes()
    for bad in ((h.scan_count(), 0, np.eye(3, 4)), (0, -1, np.eye(3, 4)), (0, 1, np.full((3, 4), np.nan))):
        with pytest.raises(capi.UzlError) as err:
            h.estimate([pair("room", 0), bad])
        assert err.value.status == capi.UZL_ERR_BAD_ARG
    with pytest.raises(capi.UzlError) as err:
        h.add_scans([dict(LS.empty_scan(), values=np.zeros(7, np.float32))])
    assert err.value.status == capi.UZL_ERR_BAD_ARG
    assert h.scan_count() == n0 + 1 and h.estimate([pair("room", 1)]).tobytes() == before


def room_images():
    """two 32 x 24 depth images of the 6 x 4 m room from two poses of a level camera 0.5 m up"""
    w, hgt = 32, 24
    fx = LLS.FX * w / 640.0
    poses = [(2.0, 1.5, 0.1), (2.1, 1.55, 0.16)]
    T = LLS.camera_transform(yaw=0.0, height=0.5)
    return [LLS.image(LS.depth_image(LS.ROOM, p, w, hgt, fx, (w - 1) / 2.0), T, group=k) for k, p in enumerate(poses)]


@pytest.mark.parametrize("use_near", [0, 1])
def test_from_depth_images(capi, use_near):
    """extract -> to_laser -> estimate = read -> add_scans -> estimate, bit for bit"""
    line = capi.Laserline()
    ranges, intensities, _ = line.extract(room_images())
    values = ranges if use_near else intensities
    lo, hi = np.float32(line.cfg.range_min), np.float32(line.cfg.range_max)
    assert 20 <= ((values[0] >= lo) & (values[0] <= hi)).sum() <= 40
    guessed = LS.pose_matrix(0.12, 0.03, 0.05)
    device, host = capi.Laser(fail_fraction=0.01), capi.Laser(fail_fraction=0.01)
    device.add_scans([SCENES["closet37"]["scan_from"]])                     # the appended scans are not the store's first
    host.add_scans([SCENES["closet37"]["scan_from"]])
    assert line.to_laser(device, use_near=bool(use_near)) == 1 and device.scan_count() == 3
    amin, inc = float(np.float32(-math.pi)), float(np.float32(line.cfg.angle_increment))
    assert host.add_scans([dict(values=v, angle_min=amin, angle_increment=inc, range_min=lo, range_max=hi) for v in values]) == 1
    pairs = [(1, 2, guessed), (2, 1, np.eye(3, 4)), (1, 1, np.eye(3, 4))]
    a, b = device.estimate(pairs), host.estimate(pairs)
    assert a.tobytes() == b.tobytes()
    assert a[0]["iterations"] >= 1 and a[2]["status"] == capi.LASER_OK and a[2]["nvalid"] == a[2]["scan_valid"]
    x = device.correspondences(1, 2, (0.12, 0.03, 0.05), 720)
    y = host.correspondences(1, 2, (0.12, 0.03, 0.05), 720)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)) and x[2].sum() > 0
    with pytest.raises(capi.UzlError) as err:
        capi.Laserline().to_laser(device)
    assert err.value.status == capi.UZL_ERR_STATE
    for hnd in (line, device, host):
        hnd.close()


def test_into_the_solver(capi, store):
    """a 4-node graph whose only loop closure is a returned laser edge: accepted by capi.Pgo, and the solve lowers chi2 from where
    odometry alone leaves it"""
    h, _ = store
    s = SCENES["room"]
    gt = [(2.0, 1.5, 0.1), (2.3, 1.4, 0.2), (2.5, 1.6, 0.3), (2.6, 1.9, 0.45)]            # node 0 and 3: the room scene's poses
    drift = (0.04, -0.03, math.radians(1.5))
    odo = []
    for a, b in zip(gt[:-1], gt[1:]):
        r = LS.relative(a, b)
        odo.append(LS.pose_matrix(r[0] + drift[0], r[1] + drift[1], r[2] + drift[2]))

    def mul(A, B):
        out = np.zeros((3, 4))
        out[:, :3] = A[:, :3] @ B[:, :3]
        out[:, 3] = A[:, :3] @ B[:, 3] + A[:, 3]
        return out

    poses = [LS.pose_matrix(*gt[0])]
    for T in odo:
        poses.append(mul(poses[-1], T))
    inv0 = np.zeros((3, 4)); inv0[:, :3] = poses[0][:, :3].T; inv0[:, 3] = -poses[0][:, :3].T @ poses[0][:, 3]
    first_guess = mul(inv0, poses[3])
    k = NAMES.index("room")
    e = h.estimate([(2 * k, 2 * k + 1, first_guess)])[0]
    assert e["status"] == capi.LASER_OK and e["matching_score"] > 0
    T = e["transform"].reshape(3, 4)
    assert math.hypot(T[0, 3] - s["true"][0], T[1, 3] - s["true"][1]) < 1e-3
    odom_info = np.diag([400.0] * 6)                                        # 0.05 m, 0.05 rad: the drift above is within it
    eye = np.eye(3, 4).reshape(12)
    n_e = 4
    edges = {"from": np.array([0, 1, 2, 0], np.int32), "to": np.array([1, 2, 3, 3], np.int32),
             "type": np.array([1, 1, 1, 105], np.int32), "sensor_from": np.zeros(n_e, np.int32), "sensor_to": np.zeros(n_e, np.int32),
             "valid": np.ones(n_e, np.int32), "transform": np.stack([t.reshape(12) for t in odo] + [e["transform"]]),
             "displacement_from": np.tile(eye, (n_e, 1)), "displacement_to": np.tile(eye, (n_e, 1)),
             "information": np.stack([odom_info.reshape(36)] * 3 + [e["information"]])}
    p = capi.Pgo(device=0)
    p.add_graph(np.stack([q.reshape(12) for q in poses]), np.array([1, 0, 0, 0], np.int32), edges)
    st = p.optimize(10)
    solved, _, used = p.store()
    p.close()
    assert used.all()
    assert st["chi2_initial"] > 1.0 and st["chi2_final"] < st["chi2_initial"]
    before = math.hypot(poses[3][0, 3] - gt[3][0], poses[3][1, 3] - gt[3][1])
    after = math.hypot(solved[3].reshape(3, 4)[0, 3] - gt[3][0], solved[3].reshape(3, 4)[1, 3] - gt[3][1])
    print("node 3: %.3f m from the truth by odometry, %.3f m after the solve; chi2 %.3f -> %.3f" % (before, after, st["chi2_initial"], st["chi2_final"]))
    assert after < before
