"""tests/radius_reference.py (float64 NumPy restatement of the uzl_radius_* contract) against the CPU checker on clouds whose
relative rotations reach 180 degrees, where the Eigen 3.2 angle and the plain rotation angle part ways (CPU)."""
import numpy as np
import pytest

import radius_reference as RR
import radius_scenes as RS

S = RS.S


def test_angle_is_theta_or_its_complement():
    rng = np.random.default_rng(11)
    R = RS.random_rotations(rng, 4000)
    flipped = RR.check_angle_property(R)
    assert 0.2 < flipped < 0.8                                    # the second branch decides often: this data reaches it
    # small rotations, the identity and exact half turns
    small = RS.random_rotations(rng, 200); small = np.einsum("nij,njk->nik", small, small.transpose(0, 2, 1))
    assert RR.check_angle_property(small) == 0.
    assert RR.angle_eigen32(np.eye(3))[0] == 0.
    for axis in range(3):
        d = -np.ones(3); d[axis] = 1.
        assert RR.angle_eigen32(np.diag(d))[0] == np.pi
    # a known angle on either side: 150 degrees about +z is reported as 150 or 210 depending on the sign the conversion gives w
    for deg in (150., -150.):
        c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
        a = np.rad2deg(RR.angle_eigen32(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.]]))[0])
        assert abs(a - (150. if deg > 0 else 210.)) < 1e-9
        assert abs(np.rad2deg(RR.angle_plain(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.]]))[0]) - 150.) < 1e-9


@pytest.mark.parametrize("max_rot", [30., 100., 170., 181., 360.])
def test_restatement_equals_oracle(oracle, max_rot):
    P, st = RS.cloud(600, seed=21)
    q = np.arange(600, dtype=np.int32)
    cfg = dict(radius=1.0, new_edge_time=5.0, max_rotation_deg=max_rot)
    f, t, cnt = oracle.radius_candidates(P, st, q, **cfg)
    jobs = list(zip(f.tolist(), t.tolist()))
    n = RS.check_against_restatement(jobs, P, st, q, cfg)
    assert n > 50 and cnt.sum() == len(jobs)
    plain, _, inside = RR.candidates(P, st, q, plain_angle=True, **cfg)
    if max_rot == 170.:
        # the plain-theta rule accepts more: every pair whose w came out negative has an Eigen angle above 180
        assert set(jobs) < set(plain) and len(plain) - len(jobs) > 100
    if max_rot == 181.:
        assert len(plain) > len(jobs)                              # theta < 181 always; 360 - theta < 181 only from 179 up
    if max_rot == 360.:
        assert jobs == plain and 0.8 * inside < len(jobs) <= inside   # nothing left but the time gap
    if max_rot == 30.:
        assert jobs == plain                                      # below 120 degrees the two agree


def test_strict_comparisons_on_representable_numbers(oracle):
    """0.25 m steps and 2 s stamps: radius equal to a distance and new_edge_time equal to a gap exclude that pair; no band"""
    n = 12
    P = RS.identity_nodes(np.stack([0.25 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)); st = (2 * S * np.arange(n)).astype(np.int64)
    for cfg, want in ((dict(radius=0.75, new_edge_time=5.0), []), (dict(radius=1.0, new_edge_time=6.0), []),
                      (dict(radius=1.0, new_edge_time=5.999), [(3, 6), (9, 6)]), (dict(radius=0.7500001, new_edge_time=5.0), [(3, 6), (9, 6)])):
        cfg = dict(max_rotation_deg=30.0, **cfg)
        f, t, _ = oracle.radius_candidates(P, st, [6], **cfg)
        assert list(zip(f.tolist(), t.tolist())) == want == RR.candidates(P, st, [6], **cfg)[0]
