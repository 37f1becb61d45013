"""Hand-made cases of the edge filter (TransformationFilter / EdgeCluster, transformation_filter.cpp:43-350) and the scenes of
its two kernels, shared by the three implementations: oracle.Filter (oracle/uzl_oracle_filter.c), np_reference.FilterRef and
capi.Filter (uzl_filter.hip + filter_kernels.hip).

A case is a function `case(make, oracle)`: a small script of add / remove / set_sensors / calc_valid_edges steps on filters it
creates with `make(**cfg)`, asserting the known answer after each step.  `make` returns an oracle.Filter, a RefFilter (FilterRef
behind the same method names) or a Lockstep of two of them, which plays every step into both and compares their whole state.
CASES maps names to cases.  tests/test_filter_cases_reference.py runs them on the CPU, tests/test_filter_edges_gpu.py on the handle
in lockstep with the oracle.

The scenes further down (pose chains, threshold columns, batch shapes) are plain edge lists; the CPU file asserts on the oracle
that each reaches what it is named after, the GPU file compares the handle with the oracle bit for bit."""
import functools
import math

import numpy as np

from filter_common import assert_same_state
from np_reference import FilterRef
from ransac_cases import lds_max_points, rot

S = 10**9
I12 = np.eye(3, 4).reshape(12)
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


def E(key, tf, tt, valid=0, score=1.0, **kw):
    d = dict(key=key, matching_score=score, valid=valid, sensor_from=-1, sensor_to=-1,
             stamps_from=np.atleast_1d(np.array(tf, np.int64)), stamps_to=np.atleast_1d(np.array(tt, np.int64)),
             transform=np.eye(3, 4).reshape(12), displacement_from=np.eye(3, 4).reshape(12),
             displacement_to=np.eye(3, 4).reshape(12), pose_from=np.eye(3, 4).reshape(12), pose_to=np.eye(3, 4).reshape(12))
    d.update(kw)
    return d


def line_edges(n, key0=10, from0_s=100.0, to0_s=300.0, dt_s=0.5, bad=(), valid=0, shift=(0.0, 0.0, 0.0)):
    """n edges forming one cluster; from-chain lands exactly on the to position except for `bad` (1 m off); `shift` moves every to
    position after that, so the cluster's transform is that translation"""
    out = []
    for k in range(n):
        pf = np.eye(3, 4); pf[:, 3] = [0.3 * k, 0.1 * k * k * 0.01, 0.0]
        pt = np.eye(3, 4); pt[:, 3] = [5.0 + 0.3 * k, 1.0 + 0.02 * k, 0.1 * (k % 3)]
        T = np.eye(3, 4); T[:, 3] = pt[:, 3] - pf[:, 3] + ([1.0, -1.0, 0.5] if k in bad else [0.0, 0.0, 0.0])
        pt[:, 3] += shift
        out.append(E(key0 + k, int((from0_s + dt_s * k) * S), int((to0_s + dt_s * k) * S), valid=valid, score=float(50 - k),
                     pose_from=pf.reshape(12), pose_to=pt.reshape(12), transform=T.reshape(12)))
    return out


def _line_edges(n, dt_s=0.5, bad=()):
    return line_edges(n, dt_s=dt_s, bad=bad)


# ------------------------------------------------------------------------------------------------------------
# the three implementations behind one set of method names
# ------------------------------------------------------------------------------------------------------------
def oracle_ransac(oracle, max_error, ransac_iterations, seed):
    """The `ransac` callback FilterRef takes: the oracle's estimateSVD + consensus3D (FilterRef restates the filter, not the RANSAC)."""
    def ransac(P, Q, job_id):
        res = oracle.prosac(P.T, Q.T, max_error, ransac_iterations, 1.0, do_prosac=False, seed=seed, job_id=job_id)
        ransac.last[job_id >> 20] = (res["T"].reshape(12).copy(), res["consensus"])
        _, s = oracle.consensus3d(P.T, Q.T, res["T"], max_error)
        return res["T"], s
    ransac.last = {}
    return ransac


class RefFilter:
    """np_reference.FilterRef behind the method names and return shapes of oracle.Filter / capi.Filter."""

    def __init__(self, oracle, **cfg):
        cfg.pop("device", None)
        self.r = FilterRef(**cfg)
        self._ransac = oracle_ransac(oracle, self.r.max_error, self.r.ransac_iterations, self.r.seed)

    def set_sensors(self, sensors):
        self.r.set_sensors(sensors)

    def add(self, edges):
        self.r.add(edges)

    def remove(self, keys):
        self.r.remove(keys)

    def all_edges(self):
        return self.r.all_edges()

    def valid_edges(self):
        return self.r.valid_edges()

    def calc_valid_edges(self):
        return self.r.calc_valid_edges(self._ransac)

    def clusters(self, with_eval=False):
        out = self.r.state()
        if with_eval:
            for d, c in zip(out, self.r.clusters):
                T, rc = self._ransac.last.get(c.uid, (I12.copy(), 0))
                d.update(P=np.asarray(getattr(c, "lastP", np.zeros((0, 3))), np.float64).reshape(-1, 3),
                         Q=np.asarray(getattr(c, "lastQ", np.zeros((0, 3))), np.float64).reshape(-1, 3), T=T, ransac_consensus=rc)
        return out

    def close(self):
        pass


class Lockstep:
    """Two filters played as one: every step goes into both, then clusters (with the last evaluation's P, Q, T and votes), all_edges
    and valid_edges are compared; the first one's answers are what the case sees."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.steps = 0

    def _same(self, step):
        self.steps += 1
        tag = (self.steps, step)
        assert_same_state(self.a.clusters(with_eval=True), self.b.clusters(with_eval=True), with_eval=True, tag=tag)
        assert np.array_equal(self.a.all_edges(), self.b.all_edges()), tag
        assert np.array_equal(self.a.valid_edges(), self.b.valid_edges()), tag

    def set_sensors(self, sensors):
        self.a.set_sensors(sensors); self.b.set_sensors(sensors)
        self._same("set_sensors")

    def add(self, edges):
        self.a.add(edges); self.b.add(edges)
        self._same("add")

    def remove(self, keys):
        self.a.remove(keys); self.b.remove(keys)
        self._same("remove")

    def calc_valid_edges(self):
        na, nb = self.a.calc_valid_edges(), self.b.calc_valid_edges()
        assert na == nb, (self.steps, na, nb)
        self._same("calc")
        return na

    def all_edges(self):
        return self.a.all_edges()

    def valid_edges(self):
        return self.a.valid_edges()

    def clusters(self, with_eval=False):
        return self.a.clusters(with_eval=with_eval)

    def close(self):
        self.a.close(); self.b.close()


def lockstep(make_a, make_b):
    return lambda **cfg: Lockstep(make_a(**cfg), make_b(**cfg))


def keys_of(f):
    return [[int(k) for k in c["keys"]] for c in f.clusters()]


def bounds_of(c):
    return (c["from_start_ns"], c["from_end_ns"], c["to_start_ns"], c["to_end_ns"])


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


# ------------------------------------------------------------------------------------------------------------
# the known answers that test_oracle_filter.py has held on the oracle from the start
# ------------------------------------------------------------------------------------------------------------
@case
def cluster_window_and_bounds(make, oracle):
    f = make(max_dt=5.0)
    f.add([E(1, 100 * S, 200 * S)])
    f.add([E(2, 104 * S, 203 * S)])              # inside +-5 s of both bounds -> same cluster
    f.add([E(3, 105 * S + 4 * S, 203 * S)])      # 109 - from_end(104) = 5 -> not < 5 -> new cluster
    f.add([E(4, 100 * S, 195 * S)])              # to: 195 - 200 = -5 -> not > -5 -> new cluster
    cl = f.clusters()
    assert [list(c["keys"]) for c in cl] == [[1, 2], [3], [4]]
    assert (cl[0]["from_start_ns"], cl[0]["from_end_ns"], cl[0]["to_start_ns"], cl[0]["to_end_ns"]) == (100 * S, 104 * S, 200 * S, 203 * S)
    assert cl[0]["changed"] == 1 and cl[1]["changed"] == 0
    assert list(f.all_edges()) == [1, 2, 3, 4]


@case
def merge_and_max_cluster_size(make, oracle):
    f = make(max_dt=5.0, max_cluster_size=6)
    f.add([E(1, 100 * S, 200 * S), E(2, 101 * S, 200 * S)])          # cluster A = {1,2}
    f.add([E(3, 108 * S, 200 * S), E(4, 109 * S, 200 * S)])          # cluster B = {3,4}  (108-101 = 7 >= 5)
    assert [list(c["keys"]) for c in f.clusters()] == [[1, 2], [3, 4]]
    f.add([E(5, 104 * S + S // 2, 200 * S)])                          # matches A and B -> added to A, then 3 + 2 < 6 -> merge
    cl = f.clusters()
    assert [list(c["keys"]) for c in cl] == [[1, 2, 5, 3, 4]]
    assert cl[0]["from_end_ns"] == 109 * S
    f.add([E(6, 105 * S, 200 * S)])                                   # size 5 < 6 -> joins, cluster is now full
    f.add([E(7, 105 * S, 200 * S)])                                   # size 6 not < 6 -> own cluster
    assert [c["size"] for c in f.clusters()] == [6, 1]
    # a merge that would reach the cap is refused (strict <)
    g = make(max_dt=5.0, max_cluster_size=5)
    g.add([E(1, 100 * S, 200 * S), E(2, 101 * S, 200 * S), E(3, 108 * S, 200 * S), E(4, 109 * S, 200 * S)])
    g.add([E(5, 104 * S + S // 2, 200 * S)])                          # 3 + 2 = 5 not < 5
    assert [list(c["keys"]) for c in g.clusters()] == [[1, 2, 5], [3, 4]]


@case
def consensus_counter_and_remove(make, oracle):
    f = make()
    f.add([E(1, 100 * S, 200 * S, valid=1), E(2, 101 * S, 200 * S, valid=0), E(3, 102 * S, 201 * S, valid=1)])
    assert f.clusters()[0]["consensus"] == 2
    f.remove([3])
    c = f.clusters()[0]
    assert c["consensus"] == 1 and list(c["keys"]) == [1, 2]
    f.remove([1, 2])
    assert f.clusters() == [] and len(f.all_edges()) == 0
    f.remove([99])                                                    # unknown id: no-op
    # an edge whose nodes carry two stamps each lands in the same cluster four times: counted four times (:74-76)
    f.add([E(7, [100 * S, 101 * S], [200 * S, 201 * S], valid=1)])
    c = f.clusters()[0]
    assert c["size"] == 1 and c["consensus"] == 4
    f.remove([7])
    assert f.clusters() == []


@case
def update_keeps_validity_and_stamps(make, oracle):
    f = make()
    f.add([E(1, 100 * S, 200 * S, valid=1)])
    f.add([E(1, 500 * S, 900 * S, valid=0)])                          # known id: only the stored edge / poses change
    c = f.clusters()[0]
    assert c["size"] == 1 and c["from_start_ns"] == 100 * S and list(c["valid"]) == [1] and c["consensus"] == 1
    assert len(f.clusters()) == 1


@case
def calc_valid_edges_gates_and_verdict(make, oracle):
    f = make(min_size=8.0, seed=3)
    f.add(_line_edges(7))
    assert f.calc_valid_edges() == 0                                  # size 7 < min_size
    f = make(min_size=8.0, seed=3)
    f.add(_line_edges(12, dt_s=0.1))
    assert f.calc_valid_edges() == 0                                  # spans 1.1 s < 2 s
    assert f.clusters()[0]["changed"] == 1                            # the gate leaves changed_ set
    f = make(min_size=8.0, seed=3)
    f.add(_line_edges(12, bad=(3, 7)))
    assert f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[0]
    assert c["changed"] == 0 and c["evaluations"] == 1
    assert list(c["valid"]) == [0 if k in (3, 7) else 1 for k in range(12)] and c["consensus"] == 10
    assert np.allclose(c["P"][0], c["Q"][0]) and not np.allclose(c["P"][3], c["Q"][3])
    assert f.calc_valid_edges() == 0                                  # unchanged cluster is skipped
    assert list(f.valid_edges()) == [10 + k for k in range(12) if k not in (3, 7)]      # 10 valid: not > 2*5 -> all


@case
def valid_edges_thinning(make, oracle):
    f = make(min_size=8.0, seed=5)
    f.add(_line_edges(16))
    assert f.calc_valid_edges() == 1
    assert f.clusters()[0]["consensus"] == 16
    # 16 valid > 10: best 5 by score (keys 10..14), then floor(3.2 i) for i < 4 -> sorted positions 0, 3, 6, 9, then the last
    assert list(f.valid_edges()) == [10, 11, 12, 13, 14, 16, 19, 25]


def failed_estimate_edges():
    es = []
    for k in range(4):
        pf = np.eye(3, 4); pf[:, 3] = [k, 0, 0]
        pt = np.eye(3, 4); pt[:, 3] = [k, 0.05 if k < 2 else 3.0 * k * k, 0]     # two pairs agree with the identity, two are far off
        es.append(E(k + 1, (100 + 2 * k) * S, (200 + 2 * k) * S, pose_from=pf.reshape(12), pose_to=pt.reshape(12)))
    return es


@case
def failed_ransac_falls_back_to_identity_count(make, oracle):
    """fewer than 3 consistent pairs: estimateSVD returns T = I, consensus3D(I) still counts near pairs (:275-276)"""
    f = make(min_size=2.0, max_error=0.3, seed=1)
    f.add(failed_estimate_edges())
    assert f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[0]
    assert c["ransac_consensus"] == 0
    assert np.array_equal(c["T"], np.eye(3, 4).reshape(12)) and list(c["valid"]) == [1, 1, 0, 0]


# ------------------------------------------------------------------------------------------------------------
# window boundaries (EdgeCluster::isPartOfCluster, :107-113): strict on all four bounds
# ------------------------------------------------------------------------------------------------------------
WINDOW_MAX_DT = (5.0, 2.5)
WINDOW_BASES = {"small": 100 * S, "epoch": 1_400_000_000 * S, "negative": -1_400_000_000 * S}
WINDOW_STEP = 1000 * S                  # between the seeded clusters of one filter: far outside every window


def window_probes(max_dt):
    """(side, stamp relative to the seed's first stamp, inside?) - the seed cluster spans [0, 1 s] on both sides.  A stamp at -max_dt
    of a start bound or +max_dt of an end bound is outside (strict comparisons); the other fourteen are inside."""
    D = int(max_dt * S)
    out = []
    for side in ("from", "to"):
        for bound, at in (("start", 0), ("end", S)):
            for off, inside in ((-D, bound == "end"), (-D + 1, True), (D - 1, True), (D, bound == "start")):
                out.append((side, at + off, inside))
    return out


def window_differences():
    """every (stamp - bound) difference in ns that the window cases put through the seconds formula, with the limit it meets"""
    out = set()
    for max_dt in WINDOW_MAX_DT:
        for side, rel, _ in window_probes(max_dt):
            for bound in (0, S):
                out.add((rel - bound, max_dt))
    return sorted(out)


def _window(max_dt, base):
    def run(make, oracle):
        f = make(max_dt=max_dt)
        want = []
        for i, (side, rel, inside) in enumerate(window_probes(max_dt)):
            tf0, tt0 = base + i * WINDOW_STEP, base + 50_000 * S + i * WINDOW_STEP
            k = 3 * i + 1
            f.add([E(k, tf0, tt0)])
            f.add([E(k + 1, tf0 + S, tt0 + S)])
            want.append([k, k + 1])
            assert keys_of(f) == want, (i, "seed")
            tf, tt = (tf0 + rel, tt0) if side == "from" else (tf0, tt0 + rel)
            f.add([E(k + 2, tf, tt)])
            seed = len(want) - 1
            if inside:
                want[seed].append(k + 2)
            else:
                want.append([k + 2])
            assert keys_of(f) == want, (i, side, rel, inside)
            c = f.clusters()[seed]
            if inside:
                assert bounds_of(c) == (min(tf0, tf), max(tf0 + S, tf), min(tt0, tt), max(tt0 + S, tt)), (i, side, rel)
            else:
                assert bounds_of(c) == (tf0, tf0 + S, tt0, tt0 + S), (i, side, rel)
                assert bounds_of(f.clusters()[-1]) == (tf, tf, tt, tt)
        assert len(f.all_edges()) == 3 * len(window_probes(max_dt))
    return run


for _dt in WINDOW_MAX_DT:
    for _name, _base in WINDOW_BASES.items():
        CASES["window_%s_%s" % (str(_dt).replace(".", "_"), _name)] = _window(_dt, _base)


# ------------------------------------------------------------------------------------------------------------
# full and capped clusters (:155), multi-stamp edges (:149-150)
# ------------------------------------------------------------------------------------------------------------
@case
def max_cluster_size_one(make, oracle):
    f = make(max_cluster_size=1)
    f.add([E(1, 100 * S, 200 * S), E(2, 100 * S, 200 * S), E(3, 100 * S, 200 * S)])      # size 1 is never < 1: nobody joins
    assert keys_of(f) == [[1], [2], [3]]
    f.add([E(4, 100 * S, [200 * S, 201 * S], valid=1)])               # not even the edge's own second stamp pair
    assert keys_of(f) == [[1], [2], [3], [4], [4]]
    assert [c["consensus"] for c in f.clusters()] == [0, 0, 0, 1, 1] and [c["changed"] for c in f.clusters()] == [0] * 5
    assert list(f.all_edges()) == [1, 2, 3, 4] and list(f.valid_edges()) == [4]
    f.remove([4])
    assert keys_of(f) == [[1], [2], [3]] and list(f.all_edges()) == [1, 2, 3]


@case
def cluster_fills_up_under_a_multi_stamp_edge(make, oracle):
    f = make(max_cluster_size=3)
    f.add([E(1, 100 * S, 200 * S), E(2, 101 * S, 200 * S)])
    f.add([E(3, [102 * S, 103 * S], 200 * S, valid=1)])               # first pair: 2 < 3, joins and fills; second pair: own cluster
    assert keys_of(f) == [[1, 2, 3], [3]]
    cl = f.clusters()
    assert bounds_of(cl[0]) == (100 * S, 102 * S, 200 * S, 200 * S) and bounds_of(cl[1]) == (103 * S, 103 * S, 200 * S, 200 * S)
    assert [c["consensus"] for c in cl] == [1, 1] and [c["changed"] for c in cl] == [1, 0]
    f.add([E(4, 103 * S, 200 * S)])                                   # the full cluster is passed over: joins the new one
    assert keys_of(f) == [[1, 2, 3], [3, 4]]
    f.remove([3])
    assert keys_of(f) == [[1, 2], [4]] and [c["consensus"] for c in f.clusters()] == [0, 0]


def _two_cluster_edge(**kw):
    """2 x 2 stamps: (100, 300), (100, 301) fall into one cluster, (200, 300), (200, 301) into another"""
    return E(7, [100 * S, 200 * S], [300 * S, 301 * S], **kw)


@case
def multi_stamp_edge_in_two_clusters(make, oracle):
    f = make(min_size=1.0, min_time_span=0.0)
    f.add([E(1, 101 * S, 300 * S)])
    f.add([_two_cluster_edge(valid=1, score=2.0)])
    assert keys_of(f) == [[1, 7], [7]]
    cl = f.clusters()
    assert [c["consensus"] for c in cl] == [2, 2] and [c["changed"] for c in cl] == [1, 1]
    assert bounds_of(cl[0]) == (100 * S, 101 * S, 300 * S, 301 * S) and bounds_of(cl[1]) == (200 * S, 200 * S, 300 * S, 301 * S)
    assert list(f.all_edges()) == [1, 7] and list(f.valid_edges()) == [7]          # valid in two clusters, returned once
    # update: both stored copies change (each cluster's next evaluation shows its copy)
    pf = np.eye(3, 4); pf[:, 3] = [1.0, 2.0, 3.0]
    pt = np.eye(3, 4); pt[:, 3] = [1.0, 2.125, 3.0]
    f.add([_two_cluster_edge(valid=0, pose_from=pf.reshape(12), pose_to=pt.reshape(12))])
    assert keys_of(f) == [[1, 7], [7]] and [c["consensus"] for c in f.clusters()] == [2, 2]
    assert f.calc_valid_edges() == 2
    cl = f.clusters(with_eval=True)
    assert np.array_equal(cl[0]["P"][1], [1.0, 2.0, 3.0]) and np.array_equal(cl[0]["Q"][1], [1.0, 2.125, 3.0])
    assert np.array_equal(cl[1]["P"][0], [1.0, 2.0, 3.0]) and np.array_equal(cl[1]["Q"][0], [1.0, 2.125, 3.0])
    assert [c["ransac_consensus"] for c in cl] == [0, 0]              # m < 3: T = I, the identity count decides
    assert [list(c["valid"]) for c in cl] == [[1, 1], [1]] and [c["consensus"] for c in cl] == [2, 2]
    # remove: both clusters lose it, the emptied one disappears
    f.remove([7])
    assert keys_of(f) == [[1]] and f.clusters()[0]["consensus"] == 1 and list(f.all_edges()) == [1]


# ------------------------------------------------------------------------------------------------------------
# merge (:171-197)
# ------------------------------------------------------------------------------------------------------------
def _three_way(make, cap):
    f = make(max_cluster_size=cap)
    f.add([E(1, 100 * S, 200 * S)])              # A
    f.add([E(9, 5000 * S, 200 * S)])             # D: unrelated, between A and the clusters it absorbs
    f.add([E(2, 108 * S, 200 * S)])              # B: from 8 s after A
    f.add([E(3, 104 * S, 208 * S)])              # C: to 8 s after A and B
    f.add([E(8, 9000 * S, 200 * S)])             # Z: unrelated, behind
    assert keys_of(f) == [[1], [9], [2], [3], [8]]
    f.add([E(4, 104 * S, 204 * S, valid=1)])     # within 5 s of A, B and C: matched = [0, 2, 3]
    return f


@case
def three_way_merge(make, oracle):
    f = _three_way(make, 100)
    assert keys_of(f) == [[1, 4, 3, 2], [9], [8]]                     # the loop runs from the back: C first, then B
    c = f.clusters()[0]
    assert bounds_of(c) == (100 * S, 108 * S, 200 * S, 208 * S) and c["uid"] == 0 and c["consensus"] == 1 and c["changed"] == 1
    assert [c["uid"] for c in f.clusters()] == [0, 1, 4]
    f.remove([2, 3])                                                  # their listings were repointed to A
    assert keys_of(f) == [[1, 4], [9], [8]]


@case
def three_way_merge_refused_in_the_middle(make, oracle):
    f = _three_way(make, 4)                                           # A{1,4} + C{3} = 3 < 4; then A{1,4,3} + B{2} = 4 not < 4
    assert keys_of(f) == [[1, 4, 3], [9], [2], [8]]
    assert bounds_of(f.clusters()[0]) == (100 * S, 104 * S, 200 * S, 208 * S)
    assert [c["uid"] for c in f.clusters()] == [0, 1, 2, 4]


@case
def merge_keeps_the_absorbers_copy(make, oracle):
    """Edge 7 is in A and in B; A's evaluation votes its copy out, B's copy stays valid.  A absorbs B: unordered_map::insert keeps A's
    copy (invalid), and B's counter is still added."""
    f = make(min_size=3.0, seed=3)
    f.add([E(7, [100 * S, 108 * S], 200 * S, valid=1, pose_to=_at([0.0, 5.0, 0.0]))])   # A = {7}, B = {7}; 5 m off
    f.add([E(k, (100 + k) * S, (200 + k) * S, pose_from=_at([k, k * k, 0.0]), pose_to=_at([k, k * k, 0.0])) for k in (1, 2, 3)])
    assert keys_of(f) == [[7, 1, 2, 3], [7]] and [c["consensus"] for c in f.clusters()] == [1, 1]
    assert f.calc_valid_edges() == 1                                  # B: size 1 < min_size
    c = f.clusters(with_eval=True)[0]
    assert c["ransac_consensus"] == 3 and list(c["valid"]) == [0, 1, 1, 1] and c["consensus"] == 3
    assert list(f.clusters()[1]["valid"]) == [1]
    f.add([E(5, 105 * S, 201 * S)])                                   # matches A (from [100, 103]) and B (from 108): A absorbs B
    assert keys_of(f) == [[7, 1, 2, 3, 5]]
    c = f.clusters()[0]
    assert list(c["valid"]) == [0, 1, 1, 1, 0] and c["consensus"] == 4 and c["changed"] == 1
    assert bounds_of(c) == (100 * S, 108 * S, 200 * S, 203 * S)
    assert list(f.valid_edges()) == [1, 2, 3]
    f.remove([7])                                                     # listed [A, A] now; its copy was invalid: the counter stays
    assert keys_of(f) == [[1, 2, 3, 5]] and f.clusters()[0]["consensus"] == 4


def _at(t):
    M = np.eye(3, 4); M[:, 3] = t
    return M.reshape(12)


@case
def remove_after_merge_with_a_stale_listing(make, oracle):
    """Edge 2 is listed [B, B] (two stamp pairs into B).  A absorbs B: the reference repoints only the first listing (:176-181), the
    second keeps naming the absorbed cluster.  remove(2) then takes it out of A once; what is left of B is in no list."""
    f = make()
    f.add([E(1, 100 * S, 200 * S)])                                   # A
    f.add([E(2, [108 * S, 109 * S], 200 * S, valid=1)])               # B, counted twice
    assert keys_of(f) == [[1], [2]] and f.clusters()[1]["consensus"] == 2
    f.add([E(3, 104 * S + S // 2, 200 * S)])
    assert keys_of(f) == [[1, 3, 2]]
    assert f.clusters()[0]["consensus"] == 2 and list(f.clusters()[0]["valid"]) == [0, 0, 1]
    f.add([E(2, [108 * S, 109 * S], 200 * S, valid=1, score=9.0)])    # update through both listings
    assert keys_of(f) == [[1, 3, 2]] and f.clusters()[0]["consensus"] == 2
    f.remove([2])
    assert keys_of(f) == [[1, 3]] and f.clusters()[0]["consensus"] == 1 and list(f.all_edges()) == [1, 3]
    f.add([E(2, 104 * S, 200 * S, valid=1)])                          # the key is new again
    assert keys_of(f) == [[1, 3, 2]] and f.clusters()[0]["consensus"] == 2
    f.remove([1, 2, 3])
    assert f.clusters() == [] and len(f.all_edges()) == 0


# ------------------------------------------------------------------------------------------------------------
# gates of calcValidEdges (:227-238)
# ------------------------------------------------------------------------------------------------------------
@case
def fractional_min_size(make, oracle):
    f = make(min_size=7.5, seed=3)
    f.add(line_edges(7))
    assert f.calc_valid_edges() == 0 and f.clusters()[0]["changed"] == 1          # 7 < 7.5; the gated cluster stays due
    f.add(line_edges(8)[7:])
    assert f.calc_valid_edges() == 1                                  # 8 >= 7.5, and a consensus of 8 >= 7.5 is a verdict
    c = f.clusters()[0]
    assert c["consensus"] == 8 and list(c["valid"]) == [1] * 8 and c["changed"] == 0
    g = make(min_size=7.5, seed=3)
    g.add(line_edges(8, bad=(2,)))
    assert g.calc_valid_edges() == 1                                  # evaluated, but 7 < 7.5: no verdict
    c = g.clusters()[0]
    assert c["consensus"] == 0 and list(c["valid"]) == [0] * 8 and c["evaluations"] == 1 and c["changed"] == 0


@case
def size_equal_to_min_size(make, oracle):
    f = make(min_size=8.0, seed=3)
    f.add(line_edges(8))
    assert f.calc_valid_edges() == 1 and f.clusters()[0]["consensus"] == 8
    g = make(min_size=9.0, seed=3)
    g.add(line_edges(8))
    assert g.calc_valid_edges() == 0 and g.clusters()[0]["changed"] == 1


def span_edges(from_span_ns, to_span_ns, n=8):
    """line_edges(n) with the stamps spread evenly over exactly the two spans"""
    es = line_edges(n)
    for k, e in enumerate(es):
        e["stamps_from"] = np.array([100 * S + (from_span_ns * k) // (n - 1)], np.int64)
        e["stamps_to"] = np.array([300 * S + (to_span_ns * k) // (n - 1)], np.int64)
    return es


SPAN_DIFFERENCES = (-2 * S, -(2 * S - 1))     # start - end, as calcValidEdges forms it


@case
def time_span_gate(make, oracle):
    for fs, ts, due in ((2 * S, 2 * S - 1, 0), (2 * S - 1, 2 * S, 0), (2 * S, 2 * S, 1)):
        f = make(min_size=8.0, seed=3)
        f.add(span_edges(fs, ts))
        c = f.clusters()[0]
        assert c["from_end_ns"] - c["from_start_ns"] == fs and c["to_end_ns"] - c["to_start_ns"] == ts
        assert f.calc_valid_edges() == due, (fs, ts)                  # |span| < 2 s is strict: exactly 2 s passes
        c = f.clusters()[0]
        assert c["changed"] == 1 - due and c["evaluations"] == due and c["consensus"] == 8 * due


# ------------------------------------------------------------------------------------------------------------
# verdict (:278-283)
# ------------------------------------------------------------------------------------------------------------
@case
def lower_score_keeps_the_flags(make, oracle):
    f = make(min_size=8.0, seed=3)
    f.add(line_edges(12))
    assert f.calc_valid_edges() == 1
    c = f.clusters()[0]
    assert c["consensus"] == 12 and list(c["valid"]) == [1] * 12
    worse = line_edges(13, bad=(0, 1, 2, 3, 4))
    f.add(worse[:5])                                                  # update: five edges are 1 m off now
    assert f.clusters()[0]["changed"] == 0 and f.calc_valid_edges() == 0
    f.add(worse[12:])                                                 # a new edge in the window makes the cluster due
    assert f.clusters()[0]["changed"] == 1 and f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[0]
    assert c["ransac_consensus"] == 8                                 # >= min_size, but below the counter
    assert c["consensus"] == 12 and list(c["valid"]) == [1] * 12 + [0]
    assert c["changed"] == 0 and c["evaluations"] == 2
    assert f.calc_valid_edges() == 0


@case
def equal_score_replaces_the_flags(make, oracle):
    f = make(min_size=8.0, seed=3)
    f.add(line_edges(12, bad=(3, 7)))
    assert f.calc_valid_edges() == 1
    c = f.clusters()[0]
    assert c["consensus"] == 10 and list(c["valid"]) == [0 if k in (3, 7) else 1 for k in range(12)]
    swapped = line_edges(13, bad=(5, 7, 12))
    f.add([swapped[3], swapped[5]])                                   # update: 3 fits now, 5 does not
    f.add([swapped[12]])                                              # new, and off
    assert f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[0]
    assert c["ransac_consensus"] == 10
    assert c["consensus"] == 10 and list(c["valid"]) == [0 if k in (5, 7, 12) else 1 for k in range(13)] and c["evaluations"] == 2
    assert list(f.valid_edges()) == [10 + k for k in range(13) if k not in (5, 7, 12)]


@case
def multi_stamp_counter_blocks_a_verdict(make, oracle):
    f = make(min_size=3.0, seed=3)
    es = line_edges(3, dt_s=1.5)
    es[0] = dict(es[0], valid=1, stamps_from=np.array([100 * S, 101 * S], np.int64), stamps_to=np.array([300 * S, 301 * S], np.int64))
    f.add(es)
    c = f.clusters()[0]
    assert c["size"] == 3 and c["consensus"] == 4 and list(c["valid"]) == [1, 0, 0] and c["changed"] == 1
    assert f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[0]
    assert c["ransac_consensus"] == 3                                 # all three fit: 3 >= min_size, but 3 < the counter of 4
    assert c["consensus"] == 4 and list(c["valid"]) == [1, 0, 0] and c["changed"] == 0 and c["evaluations"] == 1
    assert list(f.valid_edges()) == [10]


def noisy_edges(n, seed=5, sigma=0.04):
    """line_edges whose measured transforms are off by noise of the size of the threshold the job-id case uses: which pairs agree
    depends on the three the estimator draws"""
    rng = np.random.default_rng(seed)
    es = line_edges(n)
    for e in es:
        T = e["transform"].reshape(3, 4).copy(); T[:, 3] += rng.normal(0, sigma, 3)
        e["transform"] = T.reshape(12)
    return es


@case
def second_evaluation_draws_from_its_own_stream(make, oracle):
    cfg = dict(min_size=3.0, ransac_iterations=2, max_error=0.05, seed=21)
    f = make(**cfg)
    f.add([E(1, 0, 0)])                                               # uid 0
    es = noisy_edges(13)
    f.add(es[:12])
    assert [c["uid"] for c in f.clusters()] == [0, 1]
    assert f.calc_valid_edges() == 1
    f.add(es[12:])
    assert f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[1]
    assert c["evaluations"] == 2 and len(c["P"]) == 13

    def est(job_id):
        return oracle.prosac(c["P"].T, c["Q"].T, cfg["max_error"], cfg["ransac_iterations"], 1.0, do_prosac=False, seed=cfg["seed"], job_id=job_id)

    want = est((1 << 20) + 1)                                         # (uid << 20) + evaluations before this one
    assert want["consensus"] >= 3
    assert np.array_equal(c["T"], want["T"].reshape(12)) and c["ransac_consensus"] == want["consensus"]
    for other in ((1 << 20), 1, (2 << 20) + 1):                       # the scene tells the streams apart
        assert not np.array_equal(est(other)["T"].reshape(12), c["T"]), other


# ------------------------------------------------------------------------------------------------------------
# validEdges thinning (:287-329)
# ------------------------------------------------------------------------------------------------------------
@case
def thinning_starts_above_twice_max_edges(make, oracle):
    f = make(max_edges=3)
    f.add(line_edges(6, valid=1))
    assert list(f.valid_edges()) == [10, 11, 12, 13, 14, 15]          # 6 is not > 2 * 3: all
    f.add(line_edges(7, valid=1)[6:])
    # 7 > 6: best 3 (10, 11, 12), then floor(7/3 i) for i < 2 -> positions 0, 2 (both among the best already), then the last
    assert list(f.valid_edges()) == [10, 11, 12, 16]


@case
def thinning_with_one_edge(make, oracle):
    f = make(max_edges=1)
    f.add([E(1, 100 * S, 200 * S, valid=1, score=5.0), E(2, 101 * S, 200 * S, valid=1, score=9.0)])
    assert list(f.valid_edges()) == [1, 2]                            # 2 is not > 2
    f.add([E(3, 102 * S, 200 * S, valid=1, score=7.0)])
    assert list(f.valid_edges()) == [1, 2]                            # the best (2), no spread pick, then the last by score (1)


@case
def thinning_equal_scores_keep_insertion_order(make, oracle):
    f = make(max_edges=3)
    order = [30, 10, 20, 50, 40, 70, 60]
    f.add([E(k, (100 + i) * S // 2, 200 * S, valid=1, score=1.0) for i, k in enumerate(order)])
    assert keys_of(f) == [order]
    assert list(f.valid_edges()) == [10, 20, 30, 60]                  # best 3 = 30, 10, 20; positions 0, 2 = 30, 20; last = 60


# ------------------------------------------------------------------------------------------------------------
# update without `changed` (EdgeCluster::updateEdge, :76-84)
# ------------------------------------------------------------------------------------------------------------
@case
def update_shows_at_the_next_evaluation(make, oracle):
    f = make(min_size=8.0, seed=3)
    es = line_edges(13)
    f.add(es[:12])
    assert f.calc_valid_edges() == 1
    before = f.clusters(with_eval=True)[0]
    pf = es[0]["pose_from"].reshape(3, 4).copy(); pf[:, 3] += [0.125, 0.0, 0.0]
    pt = es[0]["pose_to"].reshape(3, 4).copy(); pt[:, 3] += [0.125, 0.0, 2.0]
    f.add([dict(es[0], pose_from=pf.reshape(12), pose_to=pt.reshape(12))])
    c = f.clusters(with_eval=True)[0]
    assert c["changed"] == 0 and f.calc_valid_edges() == 0            # an update does not make the cluster due
    assert np.array_equal(c["P"], before["P"]) and c["evaluations"] == 1
    f.add(es[12:])
    assert f.calc_valid_edges() == 1
    c = f.clusters(with_eval=True)[0]
    assert np.array_equal(c["Q"][0], pt[:, 3]) and np.array_equal(c["P"][0], es[0]["transform"].reshape(3, 4)[:, 3] + pf[:, 3])
    assert np.array_equal(c["P"][1:12], before["P"][1:]) and np.array_equal(c["Q"][1:12], before["Q"][1:])
    assert list(c["valid"]) == [0] + [1] * 12 and c["consensus"] == 12             # 2 m off in z now


# ------------------------------------------------------------------------------------------------------------
# seconds between two stamps: the contract's formula and ros::Duration::toSec()
# ------------------------------------------------------------------------------------------------------------
def contract_seconds(d_ns):
    """(double)(a - b) * 1e-9, as uzl_filter.hip, the oracle and FilterRef compute it"""
    return float(d_ns) * 1e-9


def ros_seconds(d_ns):
    """ros::Duration(a - b).toSec(): normalised to sec = floor(d / 1e9), 0 <= nsec < 1e9, then (double)sec + 1e-9 * (double)nsec"""
    sec, nsec = divmod(int(d_ns), S)
    return float(sec) + 1e-9 * float(nsec)


# ------------------------------------------------------------------------------------------------------------
# scenes of filter_points_kernel: one cluster of a dozen edges, each a chain of five isometries
# ------------------------------------------------------------------------------------------------------------
def iso(R, t):
    M = np.zeros((3, 4)); M[:, :3] = R; M[:, 3] = t
    return M.reshape(12)


def to44(m12):
    M = np.eye(4); M[:3] = np.asarray(m12, np.float64).reshape(3, 4)
    return M


CHAIN_CFG = dict(min_size=8.0, ransac_iterations=100, max_error=0.3, seed=12)
CHAIN_N = 12
CHAIN_KINDS = ("index_2_and_5", "index_minus_2", "index_int32_extremes", "no_sensors", "near_half_turn", "far", "one_sided", "nan_pose")


def _sensor_index(kind, k):
    if kind == "index_2_and_5":
        return (0, 1, 2, 5)[k % 4], (5, 2, 1, 0)[k % 4]
    if kind == "index_minus_2":
        return (-2, 0, 1, -1)[k % 4], (1, -2, -2, 0)[k % 4]
    if kind == "index_int32_extremes":
        return (INT32_MAX, INT32_MIN, 0, 1)[k % 4], (1, INT32_MAX, INT32_MIN, 0)[k % 4]
    return k % 2, (k // 2) % 2


@functools.lru_cache(maxsize=None)
def chain_scene(kind):
    """dict(sensors (n,12), edges): the `to` end is placed where the float64 chain of the `from` end lands (k = 3 and 8 one metre off),
    so the estimate is the identity and succeeds."""
    rng = np.random.default_rng(40 + CHAIN_KINDS.index(kind))
    half = kind == "near_half_turn"
    scale = 1e6 if kind == "far" else 1.0
    ax = np.eye(3)

    def R(k):
        return rot(ax[k % 3] * (np.pi - 1e-6 * rng.uniform(0.1, 1.0))) if half else rot(rng.normal(0, 1.2, 3))

    sensors = np.array([iso(R(0), rng.uniform(-0.5, 0.5, 3)), iso(R(2), rng.uniform(-0.5, 0.5, 3))])
    if kind == "no_sensors":
        sensors = np.zeros((0, 12))
    edges = []
    for k in range(CHAIN_N):
        sf, st = _sensor_index(kind, k)
        pose_from = iso(R(k), rng.uniform(-5, 5, 3) * scale)
        disp_from = iso(R(k + 1), rng.uniform(-0.3, 0.3, 3))
        transform = iso(R(k + 2), rng.uniform(-2, 2, 3) * scale)
        Rto, disp_to = R(k), iso(R(k + 1), rng.uniform(-0.3, 0.3, 3))
        if kind == "one_sided":
            if k % 2:
                disp_from = I12.copy()
            else:
                disp_to = I12.copy()
        chain = to44(pose_from) @ to44(disp_from)
        for m in (sensors[sf] if 0 <= sf < len(sensors) else I12, transform):
            chain = chain @ to44(m)
        chain = chain @ np.linalg.inv(to44(sensors[st] if 0 <= st < len(sensors) else I12))
        p = chain[:3, 3] + (np.array([1.0, -1.0, 0.5]) if k in (3, 8) else 0.0)
        pose_to = iso(Rto, p - Rto @ disp_to.reshape(3, 4)[:, 3])
        if kind == "nan_pose" and k == 4:
            pose_from = pose_from.copy(); pose_from[3] = np.nan
        edges.append(E(10 + k, int((100 + 0.5 * k) * S), int((300 + 0.5 * k) * S), score=float(50 - k), sensor_from=sf, sensor_to=st,
                       pose_from=pose_from, pose_to=pose_to, transform=transform, displacement_from=disp_from, displacement_to=disp_to))
    return dict(sensors=sensors, edges=edges)


@functools.lru_cache(maxsize=None)
def sensor_tables():
    """two sensors, two other sensors, none - and 14 edges that use indices 0 and 1: twelve for the first evaluation, one more for each
    of the next two"""
    rng = np.random.default_rng(77)
    tabs = [np.array([iso(rot(rng.normal(0, 1, 3)), rng.uniform(-1, 1, 3)) for _ in range(2)]) for _ in range(2)] + [np.zeros((0, 12))]
    edges = []
    for k in range(14):
        pf = iso(rot(rng.normal(0, 1, 3)), rng.uniform(-5, 5, 3))
        tr = iso(rot(rng.normal(0, 1, 3)), rng.uniform(-2, 2, 3))
        edges.append(E(10 + k, int((100 + 0.25 * k) * S), int((300 + 0.25 * k) * S), sensor_from=k % 2, sensor_to=(k + 1) % 2,
                       pose_from=pf, transform=tr, pose_to=iso(np.eye(3), rng.uniform(-5, 5, 3))))
    return tabs, edges


def chain_longdouble(e, sensors):
    """The two translations of one edge as the plain product of 4 x 4 matrices in numpy.longdouble, with the general inverse of the
    `to` sensor (numpy.linalg.inv, polished by one Newton step in long double: linalg itself stops at float64), and the sum of the
    magnitudes of the translation terms of each product.  An index outside the table is the identity (the contract's choice)."""
    L = np.longdouble

    def M(m12):
        return to44(m12).astype(L)

    def sensor(i):
        return np.asarray(sensors[i] if 0 <= i < len(sensors) else I12, np.float64)

    St = M(sensor(e["sensor_to"]))
    X = np.linalg.inv(St.astype(np.float64)).astype(L)
    X = X @ (2 * np.eye(4, dtype=L) - St @ X)
    fa = [M(e["pose_from"]), M(e["displacement_from"]), M(sensor(e["sensor_from"])), M(e["transform"]), X]
    fb = [M(e["pose_to"]), M(e["displacement_to"])]
    out = []
    for fs in (fa, fb):
        prod = fs[0]
        for m in fs[1:]:
            prod = prod @ m
        out.append((prod[:3, 3], sum(np.sqrt(np.sum(m[:3, 3] ** 2)) for m in fs)))
    return out


# ------------------------------------------------------------------------------------------------------------
# scenes of filter_consensus_kernel: columns at the threshold
# ------------------------------------------------------------------------------------------------------------
THRESHOLD = 0.25                         # sqrt(0.0625) is exact
THRESHOLD_OFFSETS = {"at": (0.0, 0.25, 0.0), "below": (0.0, math.nextafter(0.25, 0.0), 0.0), "above": (0.0, math.nextafter(0.25, 1.0), 0.0),
                     "3-4-5": (0.15, 0.2, 0.0)}
THRESHOLD_FAILED_CFG = dict(min_size=1.0, max_error=THRESHOLD, seed=1)
THRESHOLD_FIT_CFG = dict(min_size=8.0, max_error=THRESHOLD, seed=2)


def threshold_failed_edges():
    """One cluster per offset, the shape of failed_estimate_edges: column 0 has Q - P = the offset, column 1 is 0.05 from the identity,
    columns 2 and 3 are far off and fit no rigid motion with the others, so the estimate fails and T = I."""
    out = []
    for c, d in enumerate(THRESHOLD_OFFSETS.values()):
        for k in range(4):
            q = d if k == 0 else ([k, 0.05, 0.0] if k == 1 else [k, 3.0 * k * k, 0.0])
            out.append(E(100 * c + k + 1, (1000 * c + 100 + 2 * k) * S, (1000 * c + 200 + 2 * k) * S, pose_from=_at([k, 0.0, 0.0]), pose_to=_at(q)))
    return out


def threshold_fit_edges():
    """Nine pairs that a translation of (2, -1, 0.5) fits exactly, then three displaced along y by the three distances."""
    pts = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 0), (4, 0, 4), (0, 4, 4), (4, 4, 4), (2, 1, 3), (1, 3, 2), (3, 2, 1), (1, 1, 1)]
    t = np.array([2.0, -1.0, 0.5])
    out = []
    for k, p in enumerate(pts):
        d = (0.0, 0.0, 0.0) if k < 9 else list(THRESHOLD_OFFSETS.values())[k - 9]
        out.append(E(10 + k, int((100 + 0.5 * k) * S), int((300 + 0.5 * k) * S), pose_from=_at(p), pose_to=_at(np.array(p, float) + t + np.array(d))))
    return out


# ------------------------------------------------------------------------------------------------------------
# batch shapes of one calc_valid_edges call
# ------------------------------------------------------------------------------------------------------------
BATCH_CFG = dict(min_size=1.0, min_time_span=0.0, ransac_iterations=50, max_error=0.3, seed=4)
BATCH_SHAPES = {63: (62, 1), 64: (1, 2, 61), 65: (3, 62), 129: (1, 62, 61, 3, 2)}       # total columns -> cluster sizes in order
MANY_SMALL = (3,) * 300


def batch_edges(sizes, first_cluster=0):
    """One cluster per size, each in a time window of its own.  A cluster of one edge is due only through addEdge, so that edge has
    two `to` stamps (both pairs fall into its cluster).  Every seventh edge from the fourth is 1 m off.  A cluster of three or more has
    a translation of its own, metres away from its neighbours': a column voted under the transform next door gets another verdict."""
    out = []
    for c, n in enumerate(sizes, first_cluster):
        shift = np.array([0.7, -0.4, 0.9]) * (1 + c % 5) if n >= 3 else np.zeros(3)
        es = line_edges(n, key0=1000 * c, from0_s=1000.0 * c, to0_s=1000.0 * c + 300.0, dt_s=4.0 / n, bad=range(3, n, 7), shift=shift)
        if n == 1:
            es[0]["stamps_to"] = np.array([int((1000.0 * c + 300.0) * S), int((1000.0 * c + 301.0) * S)], np.int64)
        out += es
    return out


LARGE_ITERATIONS = 4096                  # the most the filter admits: the smallest LDS bound of the estimator
LARGE_M = lds_max_points(LARGE_ITERATIONS) + 1
LARGE_CFG = dict(min_size=8.0, max_cluster_size=LARGE_M + 1, ransac_iterations=LARGE_ITERATIONS, max_error=0.3, seed=6)


@functools.lru_cache(maxsize=None)
def large_edges():
    """LARGE_M edges within 2.5 s (one cluster), a fifth of them off by 1 to 3 m, then two small clusters"""
    out = []
    for k in range(LARGE_M):
        pf = [0.01 * k, math.sin(0.1 * k), math.cos(0.37 * k)]
        off = np.array([1.0, -1.0, 0.5]) * (1 + k % 3) if k % 5 == 0 else np.zeros(3)
        out.append(E(k, 100 * S + k * 10**6, 300 * S + k * 10**6, score=float(k % 97), pose_from=_at(pf), pose_to=_at(np.array(pf) + [5.0, 1.0, 0.0] + off),
                     transform=_at([5.0, 1.0, 0.0])))
    return out + batch_edges((8, 12), first_cluster=10)


def after_large_edges():
    return batch_edges((8,), first_cluster=20)
