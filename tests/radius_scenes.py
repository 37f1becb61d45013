"""Node clouds for the uzl_radius_* tests (test_radius_reference.py on the CPU, test_radius_gpu.py) and the comparison of a job list
with the restatement tests/radius_reference.py outside the threshold band."""
import numpy as np

import radius_reference as RR

S = 10**9
BAND = 1e-9                       # relative distance to a threshold within which a pair is left out of the NumPy comparison
MAX_SHARE = 0.01                  # of the pairs inside the radius


def random_rotations(rng, n):
    """uniformly random rotations (unit quaternions uniform on the 3-sphere): angles up to 180 degrees, most of them above 90"""
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def poses_of(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3, 1)], axis=2).reshape(-1, 12)


def cloud(n, seed, per_ball=30.0, radius=1.0):
    """n nodes uniform in a cube that holds about per_ball nodes per ball of `radius`, uniformly random rotations, stamps random
    nanosecond counts within 200 s -> (poses n x 12, stamps)"""
    rng = np.random.default_rng(seed)
    edge = max((n / per_ball * 4.18879 * radius**3) ** (1 / 3), 0.5 * radius)
    t = rng.uniform(0, edge, (n, 3))
    st = rng.integers(0, 200 * S, n).astype(np.int64)
    return poses_of(random_rotations(rng, n), t), st


def identity_nodes(t):
    t = np.asarray(t, np.float64).reshape(-1, 3)
    return poses_of(np.tile(np.eye(3), (len(t), 1, 1)), t)


def check_against_restatement(jobs, poses, stamps, queries, cfg, band=BAND):
    """jobs: list of (from, to) of an implementation.  Equal to the restatement's, in order, once the pairs within `band` of a
    threshold are taken out of both; at most MAX_SHARE of the pairs inside the radius may be taken out.  band = 0: nothing is."""
    want, near, inside = RR.candidates(poses, stamps, queries, band=band, **cfg)
    assert len(near) <= MAX_SHARE * max(inside, 1), (len(near), inside)
    got = [j for j in jobs if j not in near]
    want = [j for j in want if j not in near]
    assert got == want
    return len(want)
