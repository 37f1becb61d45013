"""Seeded scenes for the stage tests of one outer iteration of uzl_cloud_* (tests/test_cloud_step_reference.py on the CPU,
tests/test_cloud_step_gpu.py on the device): degenerate geometry (one exact plane, collinear kept points, 1 - 6 kept
correspondences, none), a room corner far from the origin, first guesses that turn the target by 90 and 180 degrees, and source
sizes and kept patterns at the edges of the step kernel's reduction (lane t of 256 owns rows t, t + 256, ...; 64-lane waves).
Every cloud is given as points (uzl_cloud_add_points), so the device and the restatement hold the same xyz; no cloud has more
than 1100 points.  A case is (scene, first guess G, estimate T, configuration)."""
import math

import numpy as np

import cloud_scenes as CS

f32 = np.float32
MAX_POINTS = 1100
SIZES = [20, 63, 64, 65, 255, 256, 257, 513, 1025]
# configurations a case may name: the handle's set_config arguments, and the same for cloud_reference.config
CONFIGS = {"default": dict(inner_iterations=10, max_iterations=20), "inner1": dict(inner_iterations=1, max_iterations=20),
           "inner2": dict(inner_iterations=2, max_iterations=20), "outer1": dict(inner_iterations=10, max_iterations=1)}
TRUE = CS.pose([0.03, -0.02, 0.025], np.radians([1.0, -1.5, 2.0]))      # the displacement of the sparse scenes
_cache = {}


def _grey(n, rng):
    """colours so close that the 6-D distance is the 3-D one to within 0.04"""
    return rng.integers(118, 123, (n, 3)).astype(np.uint8)


def _move(T, xyz):
    return (np.asarray(xyz, np.float64) @ T[:, :3].T + T[:, 3]).astype(f32)


def _surface(n, rng):
    """n points of a wavy sheet in front of the camera"""
    xy = rng.uniform(-0.5, 0.5, (n, 2))
    return np.stack([xy[:, 0], xy[:, 1], 1.5 + 0.1 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])], 1)


def _away(n, rng):
    """n points beyond max_correspondence_dist of everything else, wherever a step may carry them"""
    return rng.uniform(-0.3, 0.3, (n, 3)) + np.array([4.0, 0.5, 1.5])


def sparse(name, n_src, kept, seed, noise=0.01, target=None, guess=TRUE):
    """a source of n_src points of which exactly those at the indices `kept` lie near the target moved by the first guess;
    the others, and the points that fill the target up to 20, lie where nothing matches them"""
    rng = np.random.default_rng(seed)
    kept = np.asarray(kept, np.int64)
    tgt = _surface(max(len(kept), 1), rng) if target is None else np.asarray(target, np.float64)
    tgt = tgt[:max(len(kept), 1)]
    fill = max(20 - len(tgt), 0)
    to_xyz = np.concatenate([tgt, _away(fill, rng) + np.array([0.0, 3.0, 0.0])]) if fill else tgt
    src = _away(n_src, rng) - np.array([0.0, 3.0, 0.0])
    if len(kept):
        src[kept] = (tgt[:len(kept)] + rng.normal(0.0, noise, (len(kept), 3)))
    to_xyz = _move(CS.inv(guess), to_xyz)                      # the target as stored: the first guess carries it back
    return dict(name=name, cloud_from=(src.astype(f32), _grey(n_src, rng)), cloud_to=(to_xyz, _grey(len(to_xyz), rng)), kept=kept,
                guesses=[guess], poses=[np.eye(3, 4), CS.pose([0.004, -0.003, 0.002], [0.002, -0.003, 0.001])], configs=["default"])


def plane():
    """both clouds are the exact plane z = 1.5 on a 0.05 grid; first guesses and estimates displaced along and across it"""
    rng = np.random.default_rng(11)
    g = np.arange(-10, 11) * 0.05
    x, y = np.meshgrid(g, g)
    xyz = np.stack([x.ravel(), y.ravel(), np.full(x.size, 1.5)], 1).astype(f32)
    bgr = _grey(len(xyz), rng)
    return dict(name="plane", cloud_from=(xyz, bgr), cloud_to=(xyz.copy(), bgr.copy()), kept=None,
                guesses=[CS.pose([0.02, 0.01, 0.03], [0, 0, 0]), CS.pose([0.0, 0.0, 0.03], [0.01, -0.02, 0.0])],
                poses=[np.eye(3, 4), CS.pose([0.02, 0.01, 0.0], [0, 0, 0]), CS.pose([0.0, 0.0, 0.03], [0, 0, 0]),
                       CS.pose([0.015, -0.01, 0.02], [0.01, 0.005, -0.01])],
                configs=["default", "inner1", "inner2", "outer1"])


def line():
    """the kept points are collinear: 30 points of a line across the view, matched to the same line moved by the first guess"""
    t = np.arange(-15, 15) / 64.0                             # dyadic, so the f32 points are collinear exactly
    pts = np.stack([t, 0.25 * t + 0.0625, 1.5 + 0.25 * t], 1)
    s = sparse("line", 40, np.arange(30), 12, noise=0.0, target=pts)
    s["poses"] = [np.eye(3, 4), CS.pose([0.01, 0.02, -0.01], [0.01, 0.0, 0.02])]
    s["configs"] = ["default", "inner2"]
    return s


def axis():
    """the kept points lie on the camera's optical axis: a = R p has no x and y at T = I, the sum H[2][2] is an exact 0 and every
    trial is refused - the one admitted geometry found that reaches a refused Cholesky ("Cloud registration")"""
    pts = np.stack([np.zeros(8), np.zeros(8), 1.0 + 0.125 * np.arange(8)], 1)
    s = sparse("axis", 24, np.arange(8), 13, noise=0.0, target=pts, guess=CS.pose([0.0, 0.0, 0.03], [0, 0, 0]))
    s["poses"], s["configs"] = [np.eye(3, 4)], ["default", "inner2"]
    return s


def corner(name, carry):
    """every third point of the room corner (cloud_scenes 'small'), both clouds carried by `carry`"""
    base = CS.scenes()["small"]
    shift = CS.pose(carry, [0, 0, 0])
    out = dict(name=name, kept=None)
    for side in ("from", "to"):
        xyz, bgr = base["cloud_" + side]
        out["cloud_" + side] = (_move(shift, xyz[::3]), bgr[::3].copy())
    out["true"] = CS.mul(shift, CS.mul(base["true"], CS.inv(shift)))
    return out


def far():
    s = corner("far", [3.0, -1.9, 2.15])                  # the corner's centre of about (0, -0.1, 2.35) goes to about (3, -2, 4.5)
    s["guesses"] = [CS.displaced(s["true"], 0.03, 1.0)]
    s["poses"] = [np.eye(3, 4), CS.pose([0.01, -0.02, 0.005], [0.002, 0.003, -0.002])]
    s["configs"] = ["default", "outer1"]
    return s


def turned():
    """first guesses that turn the target by 90 and by 180 degrees (the stored target is turned the other way, so the moved target
    lies on the source again), and an estimate turned by 30 degrees about the cloud's centre"""
    base = corner("turned", [0.0, 0.0, 0.0])
    src = base["cloud_from"][0].astype(np.float64)
    c = src.mean(0)
    R30 = CS.rot(np.radians(30.0) * np.array([0.6, 0.0, 0.8]))
    T30 = np.concatenate([R30, (c - R30 @ c)[:, None]], 1)
    out = []
    for tag, w in (("quarter", np.array([0.0, 0.0, 1.0]) * math.pi / 2), ("half", np.array([0.6, 0.8, 0.0]) * math.pi)):
        G = CS.mul(base["true"], CS.pose([0.02, -0.01, 0.03], w))
        s = dict(base, name="turned_" + tag)
        s["cloud_to"] = (_move(CS.mul(CS.inv(G), base["true"]), base["cloud_to"][0]), base["cloud_to"][1])
        s["guesses"], s["poses"], s["configs"] = [G], [np.eye(3, 4), T30], ["default"]
        out.append(s)
    return out


def none():
    """nothing within reach: NO_CORR at the first outer iteration"""
    return sparse("none", 24, [], 17)


def scenes():
    """name -> scene: dict(cloud_from, cloud_to: (xyz f32, bgr u8); guesses; poses; configs; kept: the indices kept by construction)"""
    if _cache:
        return _cache
    made = [plane(), line(), axis(), far(), none()] + turned()
    # 1, 2, 3 and 6 kept correspondences 2 cm off: H is rank deficient.  The seeds are the first at which the restatement's whole
    # solve takes 2 outer iterations and ends LOW_SCORE, with rejected trials at 2, 3 and 6 kept and none at 1
    # (tests/test_cloud_step_reference.py asserts it)
    for k, seed in ((1, 20), (2, 23), (3, 23), (6, 21)):
        s = sparse("few%d" % k, 24, 3 + 2 * np.arange(k), seed, noise=0.02)
        s["configs"] = ["default", "inner2"] if k == 3 else ["default"]
        made.append(s)
    for n in SIZES:
        made.append(sparse("all%d" % n, n, np.arange(n), 100 + n))
    made.append(sparse("lanes192", 1025, [i for i in range(1025) if i % 256 >= 192], 201))     # the last wave only
    made.append(sparse("second_stride", 513, np.arange(256, 513), 202))                         # rows t + 256 only
    made.append(sparse("alternate", 513, np.arange(0, 513, 2), 203))
    made.append(sparse("one_wave_few", 257, np.arange(70, 75), 204))                            # fewer kept rows than a wave, in wave 1
    for s in made:
        assert s["name"] not in _cache
        for side in ("from", "to"):
            xyz, bgr = s["cloud_" + side]
            assert 20 <= len(xyz) <= MAX_POINTS and len(bgr) == len(xyz) and xyz.dtype == f32, (s["name"], side, len(xyz))
        _cache[s["name"]] = s
    return _cache


def cases():
    """every (scene name, guess index, pose index, configuration name)"""
    return [(n, g, t, c) for n, s in scenes().items() for g in range(len(s["guesses"])) for t in range(len(s["poses"])) for c in s["configs"]]
