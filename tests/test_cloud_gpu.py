"""GPU tests of uzl_cloud_* (colour point-cloud registration): steps 1-3 and the stage entry (step 6) equal the NumPy restatement
tests/cloud_reference.py bit for bit; the covariances agree within the restatement's own error; the whole solve equals it in every
integer and within a rounding of f32 in the pose; the gates; a pair's result does not depend on the batch; refined depth images go
into the store on the device as through the host; and a returned edge closes a loop in the pose-graph solver."""
import math

import numpy as np
import pytest

import cloud_reference as LR
import cloud_scenes as CS

pytestmark = pytest.mark.gpu

SCENES = CS.scenes()
NAMES = list(SCENES)
CASES = [(n, g) for n in CS.SOLVE for g in range(len(CS.GUESSES))]
# Largest |device - restatement| over the 12 entries of `transform` measured on CASES at the first GPU run: DESIGN.md, "Cloud
# registration".  It is 0: the two differ by the order of step 7's sums only (1e-16 relative in T), and transform is made of T
# rounded to f32.  Ten times the measurement is 0 as well, so the assertion allows what that rounding can turn a last-place
# difference of T into: one unit in the last place of an f32 rotation entry, 2^-23, on T_final and hence on the product.
POSE_MEASURED = 0.0
POSE_BOUND = max(10 * POSE_MEASURED, 2.0 ** -23)
# Largest |restatement in f64 - restatement in numpy.longdouble| over the entries of C (step 4) on the scenes' points that are not
# left out, measured on the CPU: DESIGN.md.  The device is held to ten times it.
COV_MEASURED = 5.068e-12
GAP, CAP = 1e-3, 0.02             # as tests/test_cloud_reference.py, which checks the cap on the CPU
_shared = {}


def guess(name, g):
    return CS.displaced(SCENES[name]["true"], *CS.GUESSES[g])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def image(s, side):
    return dict(depth=s["depth_" + side], fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], camera_transform=np.eye(3, 4))


@pytest.fixture(scope="module")
def store(capi):
    """one handle with every scene's clouds (cloud 2 k = from, 2 k + 1 = to of scene k), added as points, and the restatement's
    clouds and results, computed once"""
    h = capi.Cloud()
    if "clouds" not in _shared:
        _shared["clouds"] = {n: (LR.make_cloud(*SCENES[n]["cloud_from"]), LR.make_cloud(*SCENES[n]["cloud_to"])) for n in NAMES}
        _shared["want"] = {(n, g): LR.estimate(*_shared["clouds"][n], guess(n, g)) for n, g in CASES}
    for k, n in enumerate(NAMES):
        a, b = _shared["clouds"][n]
        assert h.add_points(a["xyz"], a["bgr"]) == 2 * k and h.add_points(b["xyz"], b["bgr"]) == 2 * k + 1
    assert h.count() == 2 * len(NAMES)
    yield h, _shared["clouds"], _shared["want"]
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_steps_1_to_3_equal_the_restatement_exactly(capi, store, name):
    _, clouds, _ = store
    s = SCENES[name]
    h = capi.Cloud()
    assert h.add_images([image(s, "from"), image(s, "to")], [s["bgr_from"], s["bgr_to"]]) == 0 and h.count() == 2
    for i, want in enumerate(clouds[name]):
        got = h.read(i)
        assert got["xyz"].shape == want["xyz"].shape
        assert np.array_equal(bits(got["xyz"]), bits(want["xyz"])) and np.array_equal(got["bgr"], want["bgr"])
        assert np.array_equal(bits(got["lab"]), bits(want["lab"]))
    h.close()


def test_image_edges(capi):
    """no valid pixel, one voxel, 16UC1, rgb8, padded rows, a 0 x 0 image: all in one call, each equal to the restatement"""
    s = SCENES["small"]
    f32 = np.float32
    nothing = np.full((4, 6), np.nan, f32)
    nothing[0, :3] = [0.0, -1.0, 7.0]
    one = np.full((2, 2), 1.0, f32)
    mm = (np.clip(s["depth_from"], 0, 6) * 1000).astype(np.uint16)
    padded = np.zeros((s["depth_to"].shape[0], s["depth_to"].shape[1] + 5), f32)[:, :-5]
    padded[:] = s["depth_to"]
    cpad = np.zeros((s["bgr_to"].shape[0], s["bgr_to"].shape[1] + 3, 3), np.uint8)[:, :-3]
    cpad[:] = s["bgr_to"]
    cam = dict(fx=1000.0, fy=1000.0, cx=-10.0, cy=-10.0, camera_transform=np.eye(3, 4))
    images = [dict(depth=nothing, **cam), dict(depth=one, **cam), dict(image(s, "from"), depth=mm), dict(image(s, "to"), depth=padded),
              dict(depth=np.zeros((0, 0), f32), **cam)]
    colors = [np.zeros((4, 6, 3), np.uint8), np.array([[[10, 20, 30], [11, 21, 32]], [[10, 20, 30], [10, 20, 30]]], np.uint8), s["bgr_from"], cpad,
              np.zeros((0, 0, 3), np.uint8)]
    h = capi.Cloud()
    assert h.add_images(images, colors) == 0 and h.count() == 5
    assert h.point_count(0) == 0 and h.point_count(4) == 0
    got = h.read(1)
    want = LR.voxel_grid(*LR.cloud_from_images(one, colors[1], 1000.0, 1000.0, -10.0, -10.0))
    assert len(want[0]) == 1 and np.array_equal(bits(got["xyz"]), bits(want[0])) and np.array_equal(got["bgr"], want[1])
    assert got["bgr"].tolist() == [[10, 20, 30]] and np.array_equal(bits(got["lab"]), bits(LR.lab(want[1])))
    d16 = (mm.astype(np.float64) * 0.001).astype(f32)
    for i, depth, col in ((2, d16, s["bgr_from"]), (3, s["depth_to"], s["bgr_to"])):
        want = LR.voxel_grid(*LR.cloud_from_images(depth, col, s["fx"], s["fy"], s["cx"], s["cy"]))
        got = h.read(i)
        assert np.array_equal(bits(got["xyz"]), bits(want[0])) and np.array_equal(got["bgr"], want[1]) and len(want[0]) > 1000
    # rgb8: the channels are swapped on upload
    assert h.add_images([image(s, "to")], [s["bgr_to"][:, :, ::-1]], encoding=capi.COLOR_RGB8) == 5
    a, b = h.read(5), h.read(3)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("xyz", "bgr", "lab"))
    # a cloud too small for step 4 is stored but cannot be registered; a grid that overflows int32 is refused
    with pytest.raises(capi.UzlError) as e:
        h.estimate([(1, 3, np.eye(3, 4))])
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    tiny = capi.Cloud(leaf_size=1e-6)
    with pytest.raises(capi.UzlError) as e:
        tiny.add_images([image(s, "to")], [s["bgr_to"]])
    assert e.value.status == capi.UZL_ERR_BAD_ARG and tiny.count() == 0
    with pytest.raises(capi.UzlError) as e:
        h.add_images([image(s, "to")], [s["bgr_from"][:-1]])
    assert e.value.status == capi.UZL_ERR_BAD_ARG and h.count() == 6
    tiny.close()
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_step_4_covariances(capi, store, name):
    h, clouds, _ = store
    k = NAMES.index(name)
    worst = 0.0
    for i, want in enumerate(clouds[name]):
        idx, _ = LR.knn(want["xyz"], 20)
        w = np.linalg.eigvalsh(LR.full(LR.neighbour_cov(want["xyz"], idx)))
        out = (w[:, 1] - w[:, 0]) < GAP * w[:, 2]
        assert out.mean() <= CAP
        got = h.read(2 * k + i)["cov"]
        assert np.array_equal(got, got.transpose(0, 2, 1))
        worst = max(worst, float(np.abs(got - LR.full(want["cov"]))[~out].max()))
    print("%s: covariances differ from the restatement by at most %.3e" % (name, worst))
    assert worst <= 10 * COV_MEASURED


def check_stage(h, ia, ib, a, b, G, T):
    got = h.correspondences(ia, ib, G, T)
    want = LR.correspondences(a, b, G, T)
    for x, y, what in zip(got, want, ("j", "dist2", "kept")):
        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), (what, np.flatnonzero(bits(x) != bits(y))[:8].tolist())
    return want


@pytest.mark.parametrize("name", NAMES)
def test_stage_equals_the_restatement_exactly(capi, store, name):
    h, clouds, _ = store
    k = NAMES.index(name)
    a, b = clouds[name]
    kept = 0
    for g in range(len(CS.GUESSES)):
        for T in (np.eye(3, 4), CS.pose([0.01, -0.02, 0.005], [0.01, 0.02, -0.01]), CS.pose([-0.06, 0.03, 0.04], [-0.03, 0.01, 0.05])):
            kept += int(check_stage(h, 2 * k, 2 * k + 1, a, b, guess(name, g), T)[2].sum())
    assert kept > 1000


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32) + np.float32([0, 0, 1.5]), rng.integers(100, 140, (n, 3)).astype(np.uint8)   # colours close enough to be matched


def test_stage_at_the_sizes_where_the_kernel_changes_path(capi):
    """a target of exactly one LDS tile (1024) and of one point more, a source of 257 points (two workgroups, one lane in the
    second), a cloud of exactly 20 points"""
    h = capi.Cloud()
    sizes = [1024, 1025, 257, 20]
    raw = [random_cloud(n, 10 + n) for n in sizes]
    raw[1][0][1024], raw[1][1][1024] = raw[2][0][0], raw[2][1][0]          # the point behind the tile lies on point 0 of the 257
    made = [LR.make_cloud(*c) for c in raw]
    for c in made:
        h.add_points(c["xyz"], c["bgr"])
    G = CS.pose([0.02, -0.01, 0.03], [0.02, -0.03, 0.01])
    T = CS.pose([0.01, 0.0, -0.01], [0.0, 0.01, 0.0])
    seen = 0
    for ia, ib in ((2, 0), (2, 1), (0, 1), (1, 0), (3, 1), (2, 3), (3, 3)):
        seen += int(check_stage(h, ia, ib, made[ia], made[ib], G, T)[2].sum())
    want = check_stage(h, 2, 1, made[2], made[1], np.eye(3, 4), np.eye(3, 4))
    assert want[0][0] == 1024 and want[1][0] == 0 and want[2][0] == 1      # the point behind the tile is found
    assert seen > 100
    for i, c in enumerate(made):                                            # the 3-D search at the same sizes
        assert np.abs(h.read(i)["cov"] - LR.full(c["cov"])).max() <= 10 * COV_MEASURED
    e = h.estimate([(2, 0, G), (3, 3, np.eye(3, 4))])
    w = [LR.estimate(made[2], made[0], G), LR.estimate(made[3], made[3], np.eye(3, 4))]
    for x, y in zip(e, w):
        assert (x["status"], x["iterations"]) == (y["status"], y["iterations"])
        assert x["num_corr_iter"][:len(y["num_corr_iter"])].tolist() == y["num_corr_iter"]
    assert e[1]["status"] == capi.CLOUD_OK and e[1]["num_corr"] == 20 and e[1]["match_score"] == 1.0
    h.close()


def test_a_tie_goes_to_the_lower_index(capi):
    """a query exactly equidistant from two targets of its colour"""
    f32 = np.float32
    pad_xyz, pad_bgr = random_cloud(20, 5)
    pad_xyz = pad_xyz + f32([3, 0, 0])
    grey = np.full((1, 3), 90, np.uint8)
    src = LR.make_cloud(np.concatenate([f32([[0.125, 0, 1]]), pad_xyz]), np.concatenate([grey, pad_bgr]))
    for order in ((0.0, 0.25), (0.25, 0.0)):
        tgt = LR.make_cloud(np.concatenate([pad_xyz[:5], f32([[order[0], 0, 1]]), pad_xyz[5:], f32([[order[1], 0, 1]])]),
                            np.concatenate([pad_bgr[:5], grey, pad_bgr[5:], grey]))
        h = capi.Cloud()
        h.add_points(src["xyz"], src["bgr"]); h.add_points(tgt["xyz"], tgt["bgr"])
        want = check_stage(h, 0, 1, src, tgt, np.eye(3, 4), np.eye(3, 4))
        j, d, kept = h.correspondences(0, 1, np.eye(3, 4), np.eye(3, 4))
        assert j[0] == 5 and kept[0] == 1 and d[0] == f32(0.125) * f32(0.125) and want[0][0] == 5
        h.close()


def test_no_correspondence_within_reach(capi, store):
    h, clouds, _ = store
    k = NAMES.index("small")
    far = CS.mul(SCENES["small"]["true"], CS.pose([0, 3.0, 0], [0, 0, 0]))
    want = check_stage(h, 2 * k, 2 * k + 1, *clouds["small"], far, np.eye(3, 4))
    assert want[2].sum() == 0
    e = h.estimate([(2 * k, 2 * k + 1, far)])[0]
    assert e["status"] == capi.CLOUD_NO_CORR and e["iterations"] == 0 and e["num_corr"] == 0 and e["matching_score"] == 0.0
    assert np.allclose(e["transform"].reshape(3, 4), far, atol=1e-15) and not e["information"].any()
    assert LR.estimate(*clouds["small"], far)["status"] == LR.NO_CORR


@pytest.mark.parametrize("name,g", CASES, ids=["%s-%d" % c for c in CASES])
def test_whole_solve(capi, store, name, g):
    """every integer equals the restatement; the pose within POSE_BOUND of it and within the project's bound of the truth"""
    h, _, want = store
    k = NAMES.index(name)
    e = h.estimate([(2 * k, 2 * k + 1, guess(name, g))])[0]
    w = want[(name, g)]
    n = len(w["num_corr_iter"])
    assert (e["status"], e["iterations"], e["num_corr"], e["n_from"], e["n_to"]) == (w["status"], w["iterations"], w["num_corr"], w["n_from"], w["n_to"])
    assert e["num_corr_iter"][:n].tolist() == w["num_corr_iter"] and not e["num_corr_iter"][n:].any()
    diff = float(np.abs(e["transform"].reshape(3, 4) - w["transform"]).max())
    dt, dr = CS.pose_errors(e["transform"], SCENES[name]["true"])
    print("%s guess %d: %d iterations, %s; |device - restatement| %.3e; %.3e m %.3e rad from the truth"
          % (name, g, e["iterations"], w["num_corr_iter"], diff, dt, dr))
    assert diff <= POSE_BOUND
    assert e["match_score"] == w["match_score"] and e["matching_score"] == 1.0 and e["status"] == capi.CLOUD_OK
    assert np.array_equal(e["information"].reshape(6, 6), np.diag([1e4] * 3 + [1e6] * 3))
    assert dt < 1e-3 and dr < 1e-4


def test_gates(capi, store):
    h, clouds, _ = store
    # a pair rendered 1.5 m apart: too little of one view lies in the other
    s = CS.make("apart", CS.pose([0, 0, 1.5], [0, 0, 0]))
    a, b = LR.make_cloud(*s["cloud_from"]), LR.make_cloud(*s["cloud_to"])
    g = capi.Cloud()
    g.add_points(a["xyz"], a["bgr"]); g.add_points(b["xyz"], b["bgr"])
    e, w = g.estimate([(0, 1, s["true"])])[0], LR.estimate(a, b, s["true"])
    assert e["status"] == w["status"] == capi.CLOUD_LOW_SCORE and e["match_score"] == w["match_score"] <= 0.3
    assert e["num_corr_iter"][:w["iterations"]].tolist() == w["num_corr_iter"] and e["matching_score"] == 0.0
    # a first guess 1.2 m off a solvable pair: TOO_FAR if the solve walks back, else whatever the restatement meets first
    k = NAMES.index("small")
    s = SCENES["small"]
    off = CS.mul(s["true"], CS.pose([1.2, 0, 0], [0, 0, 0]))
    e, w = h.estimate([(2 * k, 2 * k + 1, off)])[0], LR.estimate(*clouds["small"], off)
    assert e["status"] == w["status"] != capi.CLOUD_OK and e["num_corr_iter"][:len(w["num_corr_iter"])].tolist() == w["num_corr_iter"]
    if CS.pose_errors(w["transform"], s["true"])[0] < 0.2:
        assert e["status"] == capi.CLOUD_TOO_FAR
    # the gate itself, at limits a solvable pair exceeds
    near = guess("small", 1)
    ia, ib = g.add_points(clouds["small"][0]["xyz"], clouds["small"][0]["bgr"]), g.add_points(clouds["small"][1]["xyz"], clouds["small"][1]["bgr"])
    for cfg, status in ((dict(max_translation=0.01), capi.CLOUD_TOO_FAR), (dict(max_rotation_deg=0.1), capi.CLOUD_TOO_FAR),
                        (dict(min_score=0.99), capi.CLOUD_LOW_SCORE), (dict(), capi.CLOUD_OK)):
        g.set_config(**dict(dict(max_translation=1.0, max_rotation_deg=30.0, min_score=0.3), **cfg))
        e = g.estimate([(ia, ib, near)])[0]
        kw = {k_: v for k_, v in cfg.items()}
        assert e["status"] == status == LR.estimate(*clouds["small"], near, LR.config(**kw))["status"]
    # 19 points are refused at add time, 20 are not
    with pytest.raises(capi.UzlError) as err:
        g.add_points(a["xyz"][:19], a["bgr"][:19])
    assert err.value.status == capi.UZL_ERR_BAD_ARG
    n = g.count()
    assert g.add_points(a["xyz"][:20], a["bgr"][:20]) == n
    g.close()


def test_a_pair_does_not_depend_on_its_batch(capi, store):
    h, _, _ = store
    k = NAMES.index("corner")
    mine = (2 * k, 2 * k + 1, guess("corner", 2))
    others = [(2 * (i % len(NAMES)) + (i % 2), 2 * ((i + 1) % len(NAMES)) + 1 - (i % 2), CS.displaced(np.eye(3, 4), 0.01 * i, 0.3 * i))
              for i in range(16)]
    others[3] = (0, 1, CS.pose([0, 3.0, 0], [0, 0, 0]))                      # one that ends at once
    alone = h.estimate([mine])[0].tobytes()
    assert h.estimate([mine] + others)[0].tobytes() == alone
    assert h.estimate(others + [mine])[-1].tobytes() == alone
    assert h.estimate(others[:8] + [mine] + others[8:])[8].tobytes() == alone
    assert h.estimate([])[:0].tobytes() == b""


def test_from_refined_depth_images(capi):
    """refine -> to_cloud leaves the store bit-equal to refine -> read -> add_images"""
    s = SCENES["corner_holes"]
    sides = ("from", "to")
    images = [image(s, side) for side in sides]
    guides = [np.ascontiguousarray(s["bgr_" + side].astype(np.uint16).sum(2) // 3).astype(np.uint8) for side in sides]
    colors = [s["bgr_" + side] for side in sides]
    f = capi.DepthFilter()
    f.refine(images, guides)
    device, host = capi.Cloud(), capi.Cloud()
    a, _ = LR.make_cloud(*SCENES["small"]["cloud_from"]), None
    device.add_points(a["xyz"], a["bgr"]); host.add_points(a["xyz"], a["bgr"])         # the appended clouds are not the store's first
    assert f.to_cloud(device, colors) == 1 and device.count() == 3
    assert host.add_images([dict(im, depth=f.read(i)) for i, im in enumerate(images)], colors) == 1
    for i in range(3):
        x, y = device.read(i), host.read(i)
        assert all(x[k].tobytes() == y[k].tobytes() for k in ("xyz", "bgr", "lab", "cov")) and (i == 0 or len(x["xyz"]) > 300)   # the filter spreads the holes
    pairs = [(1, 2, CS.displaced(s["true"], 0.03, 1.0)), (2, 1, np.eye(3, 4))]
    assert device.estimate(pairs).tobytes() == host.estimate(pairs).tobytes()
    with pytest.raises(capi.UzlError) as err:
        capi.DepthFilter().to_cloud(device, colors)
    assert err.value.status == capi.UZL_ERR_STATE
    with pytest.raises(capi.UzlError) as err:
        f.to_cloud(device, [colors[0], colors[1][:-1]])
    assert err.value.status == capi.UZL_ERR_BAD_ARG and device.count() == 3
    for hnd in (f, device, host):
        hnd.close()


def test_into_the_solver(capi, store):
    """a 4-node graph whose only loop closure is a returned cloud edge: accepted by capi.Pgo as a TYPE_3D_FULL edge, and the solve
    brings the last node closer to the truth than odometry leaves it"""
    h, _, _ = store
    k = NAMES.index("corner")
    true = SCENES["corner"]["true"]                                          # node 0 <- node 3
    steps = [CS.pose(true[:, 3] / 3, [0.0, 0.0, 0.0])] * 2
    steps.append(CS.mul(CS.inv(CS.mul(steps[0], steps[1])), true))
    gt = [np.eye(3, 4)]
    for T in steps:
        gt.append(CS.mul(gt[-1], T))
    odo = [CS.mul(T, CS.pose([0.02, -0.015, 0.01], np.radians([0.5, -0.4, 0.6]))) for T in steps]
    poses = [np.eye(3, 4)]
    for T in odo:
        poses.append(CS.mul(poses[-1], T))
    e = h.estimate([(2 * k, 2 * k + 1, CS.mul(CS.inv(poses[0]), poses[3]))])[0]
    assert e["status"] == capi.CLOUD_OK and e["matching_score"] == 1.0
    assert CS.pose_errors(e["transform"], true)[0] < 1e-3
    odom_info = np.diag([400.0] * 6)
    eye = np.eye(3, 4).reshape(12)
    n_e = 4
    edges = {"from": np.array([0, 1, 2, 0], np.int32), "to": np.array([1, 2, 3, 3], np.int32),
             "type": np.array([1, 1, 1, 1], np.int32), "sensor_from": np.zeros(n_e, np.int32), "sensor_to": np.zeros(n_e, np.int32),
             "valid": np.ones(n_e, np.int32), "transform": np.stack([t.reshape(12) for t in odo] + [e["transform"]]),
             "displacement_from": np.tile(eye, (n_e, 1)), "displacement_to": np.tile(eye, (n_e, 1)),
             "information": np.stack([odom_info.reshape(36)] * 3 + [e["information"]])}
    p = capi.Pgo(device=0)
    p.add_graph(np.stack([q.reshape(12) for q in poses]), np.array([1, 0, 0, 0], np.int32), edges)
    st = p.optimize(10)
    solved, _, used = p.store()
    p.close()
    assert used.all()
    assert st["chi2_final"] < st["chi2_initial"]
    before = CS.pose_errors(poses[3], gt[3])[0]
    after = CS.pose_errors(solved[3].reshape(3, 4), gt[3])[0]
    print("node 3: %.4f m from the truth by odometry, %.4f m after the solve; chi2 %.3f -> %.3f" % (before, after, st["chi2_initial"], st["chi2_final"]))
    assert after < before
