"""GPU tests of the four device modules that take binary descriptors of a caller-chosen width, at the widths their contracts admit
besides 32 and 64 bytes (the two with fast paths of their own): the matcher's generic 2-NN kernel alone, through the estimator and
in one batch with both matrix-core kernels; the feature repository's nearest-feature kernel at 1 and 3 chunks; binary GIST at rows
that need padding; Feature records <-> frame arena at 1-7 descriptor words per keypoint.  Every comparison is exact, against
oracle.knn2 / oracle.estimate_edge, tests/gfr_reference.py, tests/gist_reference.py and oracle/wire.py; the inputs are those of
tests/width_scenes.py, which test_descriptor_widths_reference.py checks on the CPU."""
import ctypes as C

import numpy as np
import pytest

import gfr_scenes as G
import width_scenes as WS
from gfr_reference import GfrReference
from oracle import wire as OW
from test_match_gpu import _add, _compare
from test_wire import _frame, _node
from uzliti_slam_amd import wire as W

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. matcher
@pytest.fixture(scope="module")
def matcher(capi):
    m = capi.Match(**WS.EST_CFG)
    yield m
    m.close()


def _knn2_equals_oracle(matcher, oracle, q, t):
    nq, nt = len(q), len(t)
    ff = matcher.add_frame(t, np.zeros((3, nt)), np.ones(nt, np.uint8))
    ft = matcher.add_frame(q, np.zeros((3, nq)), np.ones(nq, np.uint8))
    got = matcher.knn2(ff, ft, nq)
    want = oracle.knn2(q, t)
    matcher.remove_frame(ff); matcher.remove_frame(ft)
    for g, w, name in zip(got, want, ("idx0", "d0", "idx1", "d1")):
        assert np.array_equal(g, w), (name, np.flatnonzero(g != w)[:8])


@pytest.mark.parametrize("nq,nt", WS.KNN2_SHAPES)
@pytest.mark.parametrize("nbytes", WS.KNN2_WIDTHS)
def test_knn2_generic_widths_bit_exact(matcher, oracle, nbytes, nq, nt):
    q, t = WS.knn2_case(nq, nt, nbytes)
    _knn2_equals_oracle(matcher, oracle, q, t)


def test_knn2_largest_distance_at_508_bytes(matcher, oracle):
    """all ones against all zeros at the widest descriptor: distance 4064, the top of the packed key's 12 distance bits"""
    for q, t in WS.knn2_extreme_case(508):
        _knn2_equals_oracle(matcher, oracle, q, t)
    q, t = WS.knn2_extreme_case(508)[0]
    ff = matcher.add_frame(t, np.zeros((3, 1)), np.ones(1, np.uint8))
    ft = matcher.add_frame(q, np.zeros((3, 1)), np.ones(1, np.uint8))
    i0, d0, i1, d1 = matcher.knn2(ff, ft, 1)
    assert (i0[0], d0[0], i1[0], d1[0]) == (0, 4064, -1, -1)


@pytest.mark.parametrize("nbytes", WS.EST_WIDTHS)
def test_estimate_generic_widths_bit_exact(matcher, oracle, nbytes):
    pairs = WS.est_pairs(nbytes)
    ids = [(_add(matcher, f), _add(matcher, t)) for f, t, _ in pairs]
    res, diag = matcher.estimate(ids, job_ids=list(range(len(pairs))), max_corr=WS.EST_KP)
    for j, (f, t, T) in enumerate(pairs):
        want = WS.oracle_edge(oracle, [f], [t], j)
        assert want["ok"] == 1 and want["consensus"] > 50
        _compare(res, diag, j, want)
        assert res[j]["frame_from"] == ids[j][0] and res[j]["frame_to"] == ids[j][1]
        assert np.abs(res[j]["T"].reshape(3, 4) - T).max() < 0.05


def _same_results(a, da, b, db):
    """two uzl_edge_result records and their diagnostics rows, field by field and bit for bit"""
    for name in a.dtype.names:
        x, y = np.atleast_1d(a[name]), np.atleast_1d(b[name])
        assert x.tobytes() == y.tobytes(), name
    for key in da:
        assert np.array_equal(da[key][:a["n_corr"]], db[key][:a["n_corr"]]), key


def test_one_batch_through_all_three_knn_kernels(matcher, oracle):
    """32-byte (matrix-core, 8 words), 64-byte (matrix-core, 16 words), 20- and 48-byte (generic) pairs interleaved in one estimate call,
    a job that has to pick its same-width combos out of four, and a job without any"""
    jobs = WS.mixed_batch()
    added = {}

    def fid(f):
        if id(f) not in added:
            added[id(f)] = _add(matcher, f)
        return added[id(f)]

    ids = [([fid(x) for x in fr], [fid(x) for x in to]) for fr, to, _ in jobs]
    job_ids = [jid for _, _, jid in jobs]
    res, diag = matcher.estimate(ids, job_ids=job_ids, max_corr=WS.EST_KP)
    for j, (fr, to, jid) in enumerate(jobs):
        want = WS.oracle_edge(oracle, fr, to, jid)
        _compare(res, diag, j, want)
        assert res[j]["job_id"] == jid
        if want["frame_from"] >= 0:
            assert res[j]["frame_from"] == ids[j][0][want["frame_from"]] and res[j]["frame_to"] == ids[j][1][want["frame_to"]]
            assert fr[want["frame_from"]]["desc"].shape[1] == to[want["frame_to"]]["desc"].shape[1]
        else:
            assert res[j]["frame_from"] == -1
    assert [int(r["ok"]) for r in res] == [1] * 9 + [0]
    assert (res[8]["frame_from"], res[8]["frame_to"]) in ((ids[8][0][0], ids[8][1][1]), (ids[8][0][1], ids[8][1][0]))
    assert res[9]["frame_from"] == -1 and res[9]["n_corr"] == 0 and res[9]["consensus"] == 0
    # one call per width: the same bytes
    for group in WS.mixed_batch_groups():
        part, pdiag = matcher.estimate([ids[j] for j in group], job_ids=[job_ids[j] for j in group], max_corr=WS.EST_KP)
        for k, j in enumerate(group):
            _same_results(res[j], {key: v[j] for key, v in diag.items()}, part[k], {key: v[k] for key, v in pdiag.items()})


def test_matcher_width_limits(capi, matcher):
    before = matcher.frame_count()
    for nbytes in (0, 2, 30, 510, 512):
        with pytest.raises(capi.UzlError) as e:
            matcher.add_frame(np.zeros((4, nbytes), np.uint8), np.zeros((3, 4)), np.ones(4, np.uint8))
        assert e.value.status == capi.UZL_ERR_BAD_ARG, nbytes
        packed = capi.Match.pack_frames([(np.zeros((4, 32), np.uint8), np.zeros((3, 4)), np.ones(4, np.uint8)),
                                         (np.zeros((4, nbytes), np.uint8), np.zeros((3, 4)), np.ones(4, np.uint8))])
        with pytest.raises(capi.UzlError) as e:
            matcher.add_frames(packed)
        assert e.value.status == capi.UZL_ERR_BAD_ARG, nbytes
    assert matcher.frame_count() == before
    for nbytes in (4, 508):                                                  # ... and both ends of the range are admitted
        fid = matcher.add_frame(np.zeros((4, nbytes), np.uint8), np.zeros((3, 4)), np.ones(4, np.uint8))
        assert W.get_frame(matcher, fid)[0].shape == (4, nbytes)
        matcher.remove_frame(fid)
    assert matcher.frame_count() == before


# ------------------------------------------------------------------------------------------------ 2. global feature repository
@pytest.mark.parametrize("nbytes,cfg_name,seed", WS.GFR_CASES, ids=[f"{b}-{n}" for b, n, _ in WS.GFR_CASES])
def test_gfr_sequences_equal_the_reference(capi, nbytes, cfg_name, seed):
    steps, features, counters = G.trace(nbytes, cfg_name, seed)
    assert counters["neighbours"] >= 50 and counters["vote_ties"] >= 1 and counters["duplicate_links"] >= 1, counters
    assert counters["popcount_drops"] >= 1 and counters["at_max_minus_1"] >= 1 and counters["at_max"] >= 1, counters
    g = capi.Gfr(**G.CONFIGS[cfg_name])
    G.replay_handle(g, steps, nbytes, check=G.same_step)
    G.same_features(g, features, nbytes)
    g.close()


@pytest.mark.parametrize("F", WS.GFR_BOUNDARY_F)
@pytest.mark.parametrize("nbytes", sorted(WS.GFR_BOUNDARY))
def test_gfr_tile_and_lane_boundaries(capi, nbytes, F):
    cfg = WS.GFR_BOUNDARY[nbytes]
    planted = WS.gfr_planted(nbytes)
    g = capi.Gfr(initial_features=64, **cfg)
    r = GfrReference(**cfg)
    for f0 in range(0, F, 4096):
        assert g.add(planted[f0:min(F, f0 + 4096)], 0) == r.add(planted[f0:min(F, f0 + 4096)], 0)
    assert g.feature_count() == r.feature_count() == F                       # every row became a feature
    for pick, q, keep in WS.gfr_boundary_queries(nbytes, F):
        a = g.search(q, 100 * WS.S)
        b = r.search(q, 100 * WS.S)
        ft, di = g.last_matches()
        assert np.array_equal(ft, r.last_matches[0]) and np.array_equal(di, r.last_matches[1]), (F, len(q))
        assert np.array_equal(ft[keep], pick[keep])
        assert np.array_equal(a, b) and np.array_equal(g.last_votes(), r.last_votes)
    for f in (0, F // 2, F - 1):
        d, pl = g.get_feature(f, nbytes)
        assert np.array_equal(d, planted[f]) and np.array_equal(pl, r.get_feature(f)[1])
    g.close()


# ------------------------------------------------------------------------------------------------ 3. binary GIST
def _same_knn(g, knn):
    pl, di = g.last_knn()
    return np.array_equal(pl, knn[0]) and np.array_equal(di, knn[1])


@pytest.mark.parametrize("cfg_name", ["defaults", "clamp"])
@pytest.mark.parametrize("nbytes", WS.GIST_WIDTHS)
def test_gist_sequences_equal_the_reference(capi, nbytes, cfg_name):
    g = capi.Gist(**WS.gist_cfgs(nbytes)[cfg_name])
    for i, st in enumerate(WS.gist_trace(nbytes, cfg_name)):
        if st["op"] == "search_and_add":
            a, pa = g.search_and_add(st["desc"], st["stamp"])
            assert pa == st["place"] and np.array_equal(a, st["neighbours"]), (i, a, st["neighbours"])
            assert _same_knn(g, st["knn"]), (i, g.last_knn(), st["knn"])
        elif st["op"] == "add":
            assert g.add(st["desc"], st["stamp"]) == st["place"]
        elif st["op"] == "search":
            a = g.search(st["desc"], st["stamp"], query_place=st["query_place"])
            assert np.array_equal(a, st["neighbours"]), (i, a, st["neighbours"])
            assert _same_knn(g, st["knn"]), (i, g.last_knn(), st["knn"])
        elif st["remove"] is not None:
            g.remove(st["remove"])
        assert g.count() == st["count"]
    g.close()


def _quota_queries(g, nbytes):
    """the query of the quota scene before and after GIST_QUOTA_REMOVED go"""
    _, _, query = WS.gist_quota_scene(nbytes)
    _, (nb1, knn1), (nb2, knn2) = WS.gist_quota_trace(nbytes)
    a = g.search(query, WS.GIST_QUOTA_STAMP, query_place=WS.GIST_QUOTA_N + 80)
    assert _same_knn(g, knn1), (g.last_knn(), knn1)
    assert g.last_knn()[0].tolist() == list(WS.GIST_QUOTA_PLANTED[:10])     # the ten lowest planted places; 512 is cut
    assert np.array_equal(a, nb1)
    for p in WS.GIST_QUOTA_REMOVED:
        g.remove(p)
    a = g.search(query, WS.GIST_QUOTA_STAMP + WS.S, query_place=WS.GIST_QUOTA_N + 81)
    assert _same_knn(g, knn2), (g.last_knn(), knn2)
    assert np.array_equal(a, nb2)


@pytest.mark.parametrize("nbytes", WS.GIST_WIDTHS)
def test_gist_quota_cut_across_lane_and_chunk_boundaries(capi, nbytes):
    desc, stamps, _ = WS.gist_quota_scene(nbytes)
    adds = WS.gist_quota_trace(nbytes)[0]
    g = capi.Gist(**WS.GIST_QUOTA_CFG)
    for p in range(WS.GIST_QUOTA_N):
        a, place = g.search_and_add(desc[p], stamps[p])
        assert place == adds[p][1] and np.array_equal(a, adds[p][0]), p
        assert _same_knn(g, adds[p][2]), (p, g.last_knn(), adds[p][2])
    _quota_queries(g, nbytes)
    g.close()


@pytest.mark.parametrize("nbytes", WS.GIST_WIDTHS)
def test_gist_quota_cut_after_a_batched_append(capi, nbytes):
    desc, stamps, _ = WS.gist_quota_scene(nbytes)
    g = capi.Gist(**WS.GIST_QUOTA_CFG)
    assert g.add_batch(desc, stamps) == 0 and g.count() == WS.GIST_QUOTA_N
    _quota_queries(g, nbytes)
    g.close()


def test_gist_width_limits(capi):
    L = capi.lib()
    buf = np.zeros(300, np.uint8)
    bp = buf.ctypes.data_as(capi.c_u8p)
    st = np.zeros(2, np.int64)
    sp = st.ctypes.data_as(capi.c_i64p)
    n = C.c_int32(); idx = C.c_int32(); tot = C.c_int64()
    out = (C.c_int32 * 16)()

    def refused(g):
        for nb in (0, 257):
            assert L.uzl_gist_search_and_add(g._h, bp, nb, C.c_int64(0), 16, out, C.byref(n), C.byref(idx)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_gist_add(g._h, bp, nb, C.c_int64(0), C.byref(idx)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_gist_search(g._h, bp, nb, C.c_int64(0), -1, 16, out, C.byref(n)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_gist_add_batch(g._h, 1, bp, None, nb, sp, C.byref(idx)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_gist_search_and_add_batch(g._h, 1, bp, None, nb, sp, C.c_int64(16), out, None, C.byref(tot),
                                                   C.byref(idx)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_gist_last_error(g._h) != b""

    # a fresh handle stays fresh: the refused lengths do not become the handle's length
    g = capi.Gist(**WS.GIST_QUOTA_CFG)
    refused(g)
    assert g.count() == 0
    # a handle in use goes on as if nothing had happened (17-byte rows)
    desc, stamps, query = WS.gist_quota_scene(17)
    adds = WS.gist_quota_trace(17)[0]
    for p in range(70):
        assert g.search_and_add(desc[p], stamps[p])[1] == p
    knn = g.last_knn()
    refused(g)
    assert g.count() == 70 and _same_knn(g, knn)
    for p in range(70, 140):
        a, place = g.search_and_add(desc[p], stamps[p])
        assert place == p and np.array_equal(a, adds[p][0]) and _same_knn(g, adds[p][2])
    g.close()
    for nb in (1, 256):                                                      # both ends of the range are admitted
        h = capi.Gist(**WS.GIST_QUOTA_CFG)
        d = np.full(nb, 0xA5, np.uint8)
        assert h.search_and_add(d, 0)[1] == 0
        e = d.copy(); e[-1] ^= 0x81
        assert h.search_and_add(e, 10 * WS.S)[0].tolist() == [0]
        assert [x.tolist() for x in h.last_knn()] == [[0], [2]]
        h.close()


# ------------------------------------------------------------------------------------------------ 4. wire records <-> frame arena
@pytest.mark.parametrize("D", WS.WIRE_WIDTHS)
def test_feature_records_at_every_word_count(capi, D):
    rng = np.random.default_rng(4000 + D)
    counts = WS.wire_counts(D)
    frames = [_frame(rng, n, D) for n in counts]
    node = _node(rng, 1, frames)
    d = W.decode_node(OW.encode_node(node))
    m = capi.Match()
    ids, uv = W.add_frames_wire(m, d.sensors_c, len(counts), sensor_frame_keys=list(range(len(counts))), want_uv=True)
    assert len(set(ids)) == len(counts) and m.frame_count() == len(counts)
    assert len(uv) == sum(counts)
    row = 0
    for k, (fid, (desc, pos, valid, u), n) in enumerate(zip(ids, frames, counts)):
        gd, gp, gv = W.get_frame(m, fid)
        records = node["sensors"][k]["records"]
        if n:
            od, op, ov, ou = OW.features_unpack(records, n, D)
            assert gd.shape == (n, D) and np.array_equal(gd, od), (D, n, "descriptors")
            assert np.array_equal(gp.view(np.uint64), op.view(np.uint64)), (D, n, "positions")
            assert np.array_equal(gv, ov), (D, n, "valid")
            assert np.array_equal(uv[row:row + n], ou), (D, n, "uv")
            assert W.frame_to_wire(m, fid, None) == OW.features_pack(desc, pos, valid, None), (D, n, "records without uv")
        else:
            assert gd.shape[0] == 0 and gv.shape == (0,)
        assert W.frame_to_wire(m, fid, u if n else None) == records, (D, n, "records")
        row += n
    m.close()


def test_wire_width_limits(capi):
    rng = np.random.default_rng(5)
    m = capi.Match()
    keep = W._Keep()
    for D in (6, 512):
        desc, pos, valid, uv = _frame(rng, 5, D)
        s = dict(raw=None, sensor_type=1, stamp_sec=1, stamp_nsec=2, sensor_frame="c", displacement=np.eye(3, 4).reshape(12), descriptor_type=2,
                 n_features=5, desc_len=D, records=OW.features_pack(desc, pos, valid, uv), camera_info=None)
        assert len(s["records"]) == W.features_size(5, D)
        sens = (W.WireSensor * 1)(W._sensor_in(keep, s))
        with pytest.raises(capi.UzlError) as e:
            W.add_frames_wire(m, sens, 1)
        assert e.value.status == capi.UZL_ERR_BAD_ARG, D
    assert m.frame_count() == 0
    m.close()
