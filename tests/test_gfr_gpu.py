"""GPU tests of uzl_gfr_* (GlobalFeatureRepositoryRecognizer + PlaceRecognizer with the exact nearest-feature search): every call of
seeded sequences equals the CPU restatement tests/gfr_reference.py exactly - neighbours, place indices, the matched feature and the
nearest distance per row, the votes per place, the feature and link counts, and at the end every stored feature with its links;
the nearest feature on both sides of every tile and lane boundary; growth of the store; a type change; two handles give identical
outputs; bad arguments return their codes and leave the handle as it was."""
import ctypes as C

import numpy as np
import pytest

import gfr_scenes as G
from gfr_reference import GfrReference

S = G.S
pytestmark = pytest.mark.gpu

# seeds at which the reference's counters show the planted cases (checked in the test itself)
CASES = [(nbytes, name, 100 * nbytes + ci) for nbytes in (32, 64, 20) for ci, name in enumerate(G.CONFIGS)]


@pytest.mark.parametrize("nbytes,cfg_name,seed", CASES, ids=[f"{b}-{n}" for b, n, _ in CASES])
def test_random_sequences_equal_the_reference(capi, nbytes, cfg_name, seed):
    steps, features, counters = G.trace(nbytes, cfg_name, seed)
    assert counters["neighbours"] >= 50 and counters["vote_ties"] >= 1 and counters["duplicate_links"] >= 1, counters
    assert counters["popcount_drops"] >= 1 and counters["at_max_minus_1"] >= 1 and counters["at_max"] >= 1, counters
    g = capi.Gfr(**G.CONFIGS[cfg_name])
    G.replay_handle(g, steps, nbytes, check=G.same_step)
    G.same_features(g, features, nbytes)
    g.close()


def _targets(F):
    """feature indices at which a wrong bound would show: first, last, both sides of every power of two and of every 512-feature tile"""
    t = {0, F - 1}
    for j in range(1, 15):
        t.update((2**j - 1, 2**j))
    for m in range(1, F // 512 + 2):
        t.update((512 * m - 1, 512 * m))
    return sorted(x for x in t if 0 <= x < F)


SIZES = sorted({2**j + o for j in range(6, 13) for o in (-1, 0, 1)} | {3 * 4096 + 5})


@pytest.fixture(scope="module")
def planted():
    """3 * 4096 + 5 random 32-byte features (mutually far apart, all past the popcount rule), shared by every size"""
    return G.dense_rows(np.random.default_rng(7), SIZES[-1], 32)


@pytest.mark.parametrize("F", SIZES)
def test_tile_and_lane_boundaries(capi, planted, F):
    rng = np.random.default_rng(F)
    g = capi.Gfr(initial_features=64)
    r = GfrReference()
    for f0 in range(0, F, 4096):
        assert g.add(planted[f0:min(F, f0 + 4096)], 0) == r.add(planted[f0:min(F, f0 + 4096)], 0)
    assert g.feature_count() == r.feature_count() == F                       # every row became a feature
    targets = _targets(F)
    for rows in (1, 63, 64, 65, 255, 256, 257, 300):
        pick = [targets[(i + rows) % len(targets)] for i in range(rows)]
        q = np.stack([G.flip(rng, planted[t], rng.integers(0, 6)) for t in pick])
        q[rows // 2:rows // 2 + rows // 8] = rng.integers(0, 256, (rows // 8, 32), dtype=np.uint8)      # some rows near nothing
        a = g.search(q, 100 * S)
        b = r.search(q, 100 * S)
        ft, di = g.last_matches()
        assert np.array_equal(ft, r.last_matches[0]) and np.array_equal(di, r.last_matches[1]), (F, rows)
        keep = np.ones(rows, bool); keep[rows // 2:rows // 2 + rows // 8] = False
        assert np.array_equal(ft[keep], np.array(pick)[keep])
        assert np.array_equal(a, b) and np.array_equal(g.last_votes(), r.last_votes)
    g.close()


def test_growth(capi):
    """initial_features = 256: store and heads double three times (features pass 1024), the link arena four times"""
    cfg = dict(initial_features=256)
    seq = G.nodes(11, 32, n_nodes=120)
    steps, features, counters, r = G.replay_reference(seq, cfg)
    crossed = [next(i for i, st in enumerate(steps) if st["F"] > c) for c in (256, 512, 1024)]
    assert crossed[0] < crossed[1] < crossed[2] < len(steps) - 5 and r.link_count() > 2048
    g = capi.Gfr(**cfg)
    G.replay_handle(g, steps, 32, check=G.same_step)
    G.same_features(g, features, 32)
    g.close()


def test_type_change_clears(capi):
    seq = [s for s in G.nodes(12, 32, n_nodes=40) if s[0] in ("search_and_add", "add") and s[1] is not None]
    g = capi.Gfr(); r = GfrReference()
    for op, desc, stamp, _ in seq:
        assert g.search_and_add(desc, stamp, 2)[1] == r.search_and_add(desc, stamp, 2)[1]
    n, F2 = g.count(), g.feature_count()
    assert n == len(seq) and F2 == r.feature_count() > 500
    later = int(seq[-1][2]) + 100 * S
    for i, (op, desc, stamp, _) in enumerate(seq):                           # the same nodes as another feature type
        a, pa = g.search_and_add(desc, later + stamp, 3)
        b, pb = r.search_and_add(desc, later + stamp, 3)
        assert pa == pb == n + i and np.array_equal(a, b)                    # place indices continue
        v = g.last_votes()
        assert np.array_equal(v, r.last_votes) and not v[:n].any()           # the earlier places get no votes
        if i == 0:
            ft, di = g.last_matches()
            assert (ft == -1).all() and (di == -1).all()                     # the repository was empty
            assert g.feature_count() == r.feature_count() <= len(desc)       # ... and restarts
            assert len(a) == 0
        assert (g.feature_count(), g.link_count()) == (r.feature_count(), r.link_count())
    assert g.feature_count() == F2                                           # the same nodes build the same repository again
    G.same_features(g, [r.get_feature(f) for f in range(r.F)], 32)
    # another byte length is fine once the type changes, and fixed again afterwards
    d16 = G.dense_rows(np.random.default_rng(1), 30, 16)
    assert g.search_and_add(d16, 10**6 * S, 4)[1] == r.search_and_add(d16, 10**6 * S, 4)[1]
    assert g.feature_count() == r.feature_count() == 30
    with pytest.raises(capi.UzlError) as e:
        g.search(seq[0][1], 0, 4)
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    g.close()


def test_two_handles_give_identical_outputs(capi):
    nbytes, cfg_name, seed = CASES[4]
    steps, features, _ = G.trace(nbytes, cfg_name, seed)
    A, B = capi.Gfr(**G.CONFIGS[cfg_name]), capi.Gfr(**G.CONFIGS[cfg_name])
    a, b = G.replay_handle(A, steps, nbytes), G.replay_handle(B, steps, nbytes)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for key in x:
            if key == "matches":
                assert np.array_equal(x[key][0], y[key][0]) and np.array_equal(x[key][1], y[key][1]), i
            else:
                assert np.array_equal(x[key], y[key]), (i, key)
    assert A.feature_count() == B.feature_count() == len(features)
    for f in range(A.feature_count()):
        (da, pa), (db, pb) = A.get_feature(f, nbytes), B.get_feature(f, nbytes)
        assert np.array_equal(da, db) and np.array_equal(pa, pb), f
    A.close(); B.close()


def test_bad_arguments_leave_the_handle_untouched(capi):
    L = capi.lib()
    nbytes, cfg_name, seed = CASES[0]
    steps, features, _ = G.trace(nbytes, cfg_name, seed)
    g = capi.Gfr()
    G.replay_handle(g, steps[:150], nbytes, check=G.same_step)
    before = (g.count(), g.feature_count(), g.link_count())
    ft0, di0 = g.last_matches(); v0 = g.last_votes()
    # a wrong byte length, too many rows
    for call in (lambda: g.search_and_add(np.zeros((5, 64), np.uint8), 0), lambda: g.add(np.zeros((5, 31), np.uint8), 0),
                 lambda: g.search(np.zeros((5, 33), np.uint8), 0), lambda: g.search_and_add(np.zeros((4097, 32), np.uint8), 0),
                 lambda: g.add(np.zeros((4097, 32), np.uint8), 0), lambda: g.search(np.zeros((4097, 32), np.uint8), 0),
                 lambda: g.search_and_add(np.zeros((5, 65), np.uint8), 0, feature_type=9)):
        with pytest.raises(capi.UzlError) as e:
            call()
        assert e.value.status == capi.UZL_ERR_BAD_ARG
    # removing twice, and places never given
    live = [st["remove"] for st in steps[:150] if st["op"] == "remove" and st["remove"] is not None]
    for p in (live[0], before[0], 10**6, -1):
        with pytest.raises(capi.UzlError) as e:
            g.remove(p)
        assert e.value.status == capi.UZL_ERR_NOT_FOUND
    # NULL outputs, an unknown feature
    d = np.ascontiguousarray(steps[0]["desc"]); dp = d.ctypes.data_as(capi.c_u8p)
    n = C.c_int32()
    assert L.uzl_gfr_search_and_add(g._h, dp, len(d), nbytes, 2, C.c_int64(0), 4, None, C.byref(n), None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_search_and_add(g._h, dp, len(d), nbytes, 2, C.c_int64(0), 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_search(g._h, dp, len(d), nbytes, 2, C.c_int64(0), -1, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_search_and_add(g._h, dp, -1, nbytes, 2, C.c_int64(0), 0, None, C.byref(n), None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_get_feature(g._h, before[1], None, 0, None, None) == capi.UZL_ERR_NOT_FOUND
    assert L.uzl_gfr_get_feature(g._h, -1, None, 0, None, None) == capi.UZL_ERR_NOT_FOUND
    assert L.uzl_gfr_last_error(g._h) != b""
    assert (g.count(), g.feature_count(), g.link_count()) == before
    ft1, di1 = g.last_matches()
    assert np.array_equal(ft0, ft1) and np.array_equal(di0, di1) and np.array_equal(v0, g.last_votes())
    # ... and the handle goes on as if none of it had happened
    G.replay_handle(g, steps[150:], nbytes, check=G.same_step)
    G.same_features(g, features, nbytes)
    g.close()
