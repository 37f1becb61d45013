"""CPU tests (no GPU): the NumPy restatement of the scan-merge contract (tests/scanmerge_reference.py) against a literal
transcription of the reference's loops (graph_grid_mapper.cpp:45-133) and its atan2f index, the scenes of
tests/scanmerge_scenes.py against the cases they are named for, and merge.sensor_moves against the loop of
graph_slam_node.cpp:993-1045."""
import itertools

import numpy as np
import pytest

import laserline_reference as LR
import scanmerge_reference as R
import scanmerge_scenes as S

F32 = np.float32


def _loops(name):
    """the reference's loops over the restatement's own points and bins of a scene"""
    a, b, Dk, Dd = S.scenes()[name]
    Da, Db = R.compose(Dk, a["displacement"]), R.compose(Dd, b["displacement"])
    exp = S.expected(name)
    pts, idx = [], []
    for which, (sc, values, D) in enumerate(((a, a["ranges"], Da), (a, a["intensities"], Da), (b, b["ranges"], Db), (b, b["intensities"], Db))):
        used, qx, qy = R.projected(sc, values, D)
        pts.append(np.stack([qx[used], qy[used]], 1))
        idx.append(exp["bin"][which][used])
    return R.reference_loops(len(a["ranges"]), a["range_min"], a["range_max"], *pts, idx, b["stamp_ns"] > a["stamp_ns"])


@pytest.mark.parametrize("name", ["crowded_newer", "crowded_older", "crowded_same", "finer_b_newer", "finer_b_older", "n65_b720", "readings",
                                  "near_tenth", "cur_at_range_min", "cur_at_range_max"])
def test_the_fold_equals_the_references_loops(name):
    ranges, intensities = _loops(name)
    exp = S.expected(name)
    assert np.array_equal(ranges, exp["ranges"], equal_nan=True)
    assert np.array_equal(intensities, exp["intensities"], equal_nan=True)


@pytest.mark.parametrize("name", ["crowded_newer", "crowded_older", "crowded_same"])
def test_the_crowded_scenes_depend_on_the_order(name):
    a, b, _, _ = S.scenes()[name]
    exp = S.expected(name)
    per_bin = np.bincount(exp["bin"][R.DROP_RANGES][exp["bin"][R.DROP_RANGES] >= 0], minlength=len(a["ranges"]))
    assert (per_bin >= 3).sum() >= 32
    branches = {t[2] for t in exp["trace"]}
    assert {"take", "mean"} <= branches and ({"newer": "newer", "older": "keep", "same": "keep"}[name.split("_")[1]] in branches)
    # folding a bin's points in the opposite order gives another scan
    bb, rb = exp["bin"][R.DROP_RANGES], exp["rho"][R.DROP_RANGES]
    differs = 0
    for k in np.flatnonzero(per_bin >= 3):
        start = exp["rho"][R.KEEP_RANGES][exp["bin"][R.KEEP_RANGES] == k]
        cur = start[-1] if len(start) else a["range_max"] + F32(1.0)
        for rho in rb[bb == k][::-1]:
            cur = R.fold(cur, rho, a["range_min"], a["range_max"], True, b["stamp_ns"] > a["stamp_ns"])
        differs += cur != exp["ranges"][k]
    assert differs > 0


def test_scenes_reach_their_cases():
    sc, ex = S.scenes(), S.expected
    for name, (a, b, _, _) in sc.items():
        assert R.on_laserline_grid(a), name
    assert [len(sc["n%d" % n][0]["ranges"]) for n in (8, 63, 64, 65, 720, 4096)] == [8, 63, 64, 65, 720, 4096]
    e = ex("finer_b_newer")
    assert (np.bincount(e["bin"][R.KEEP_RANGES][e["bin"][R.KEEP_RANGES] >= 0], minlength=64) == 0).sum() >= 8        # empty bins of a
    assert np.bincount(e["bin"][R.DROP_RANGES][e["bin"][R.DROP_RANGES] >= 0], minlength=64).max() >= 32
    lo, hi = F32(S.LO), F32(S.HI)
    e = ex("cur_at_range_min")
    curs = np.array([t[0] for t in e["trace"]])
    assert (curs == lo).any() and (curs == np.nextafter(lo, F32(0))).any() and (curs == np.nextafter(lo, F32(9))).any()
    e = ex("cur_at_range_max")
    curs = np.array([t[0] for t in e["trace"]])
    assert (curs == hi).any() and (curs == np.nextafter(hi, F32(0))).any() and (curs == np.nextafter(hi, F32(9))).any()
    e = ex("near_tenth")
    d = np.array([np.abs(t[0] - t[1]) for t in e["trace"] if t[2] in ("mean", "keep")], F32)
    tenth = F32(0.1)
    assert ((d < tenth) & (d > tenth - F32(1e-6))).any() and ((d >= tenth) & (d < tenth + F32(1e-6))).any()
    assert {"mean", "keep"} <= {t[2] for t in e["trace"]}
    for name, neg in (("seam_pos_zero", False), ("seam_neg_zero", True)):
        a, b, Dk, Dd = sc[name]
        used, qx, qy = R.projected(b, b["ranges"], R.compose(Dd, b["displacement"]))
        assert used[0] and qx[0] == F32(-2.0) and qy[0] == 0 and bool(np.signbit(qy[0])) == neg, name
        assert used[3] and qx[3] == 0 and qy[3] == 0                                # the point at the origin
        e = ex(name)
        assert e["bin"][R.DROP_RANGES][0] == 63 and e["bin"][R.DROP_RANGES][3] == -1 and e["rho"][R.DROP_RANGES][3] == 0
    e = ex("readings")
    a, b, _, _ = sc["readings"]
    for which, v in ((R.KEEP_RANGES, a["ranges"]), (R.DROP_INTENSITIES, b["intensities"])):
        with np.errstate(invalid="ignore"):
            used = ~np.isnan(v) & (v >= lo) & (v <= hi)
        assert np.array_equal(e["bin"][which] >= 0, used) and used.any() and not used.all()
        assert used[v == lo].all() and used[v == hi].all() and not used[v == np.nextafter(hi, F32(9))].any()


def test_the_references_atan2f_index_differs_in_fewer_than_1_in_5000_points():
    """seeded scans of 720 beams under generic displacements (measured: 5 in 216,000 over 300 scans)"""
    rng = np.random.default_rng(2024)
    amin, amax, inc, n = LR.angular_grid(S.inc_for(720))
    ca, sa = LR.trig_table(amin, inc, n)
    total = differ = 0
    for _ in range(300):
        sc = S.room(rng, 720, holes=0.0)
        used, qx, qy = R.projected(sc, sc["ranges"], S.generic(rng))
        ours = LR.bins(qx[used], qy[used], ca, sa)
        theirs = R.reference_index(qx[used], qy[used], amin, amax, inc)
        total += int(used.sum())
        differ += int((ours != theirs).sum())
    print("atan2f index differs in %d of %d points" % (differ, total))
    assert total == 216000 and differ * 5000 < total


def test_an_identity_displacement_puts_a_on_its_bin_boundaries():
    """the divergence the header states: the reference's own index of a's points is rounding noise there, and can leave [0, n)"""
    a, _, _, _ = S.scenes()["identity"]
    used, qx, qy = R.projected(a, a["ranges"], np.eye(3, 4))
    amin, amax, inc, n = LR.angular_grid(S.inc_for(720))
    theirs = R.reference_index(qx[used], qy[used], amin, amax, inc)
    beam = np.flatnonzero(used)
    off = (theirs != beam).sum()
    print("identity: the reference's index is not the beam for %d of %d points; max index %d of n = %d" % (off, len(beam), theirs.max(), n))
    assert 0.05 * len(beam) < off < 0.95 * len(beam)
    ours = S.expected("identity")["bin"][R.KEEP_RANGES][used]
    assert ((ours == beam) | (ours == beam - 1) | ((beam == 0) & (ours == n - 1))).all()


def test_scope_and_compose():
    a, b, Dk, Dd = S.scenes()["n720"]
    assert R.on_laserline_grid(a) and not R.on_laserline_grid(S.scenes()["seam_pos_zero"][1])
    from uzliti_slam_amd import merge
    assert np.array_equal(R.compose(Dk, a["displacement"]).reshape(12), merge._compose(Dk.reshape(12), a["displacement"].reshape(12)))


# ------------------------------------------------------------------------------------- merge.sensor_moves
def _loop_of_the_reference(keep, drop):
    """graph_slam_node.cpp:993-1045 over type lists"""
    FEATURE, GIST, LASER = 1, 3, 4
    first = list(keep)
    out = []
    for t in drop:
        if t == LASER:
            exists = False
            for i in range(len(first)):
                if first[i] == LASER:
                    out.append(("merge", i)); exists = True
                    break
            if not exists:
                first.append(t); out.append(("move", len(first) - 1))
        elif t == FEATURE:
            exists = any(x == FEATURE for x in first)
            if not exists:
                first.append(t); out.append(("move", len(first) - 1))
            else:
                out.append(("discard", -1))
        elif t == GIST:
            exists = any(x == GIST for x in first)
            if not exists:
                first.append(t); out.append(("move", len(first) - 1))
            else:
                out.append(("discard", -1))
        else:
            out.append(("discard", -1))
    return out


def test_sensor_moves_on_every_combination_the_loop_distinguishes():
    from uzliti_slam_amd import merge as M
    assert (M.SENSOR_TYPE_FEATURE, M.SENSOR_TYPE_BINARY_GIST, M.SENSOR_TYPE_LASERSCAN) == (1, 3, 4)
    types = (1, 2, 3, 4)                                     # 2 = a depth image: none of the three, never moved
    keeps = [c for k in range(0, 4) for c in itertools.permutations(types, k)]
    drops = [c for k in range(0, 4) for c in itertools.product(types, repeat=k)]
    for keep in keeps:
        for drop in drops:
            assert M.sensor_moves(keep, drop) == _loop_of_the_reference(keep, drop), (keep, drop)
    # the named cases
    assert M.sensor_moves([1, 4], [4]) == [(M.SENSOR_MERGE, 1)]
    assert M.sensor_moves([1], [4, 4]) == [(M.SENSOR_MOVE, 1), (M.SENSOR_MERGE, 1)]      # the second merges into the one just moved
    assert M.sensor_moves([1, 3], [1, 3]) == [(M.SENSOR_DISCARD, -1)] * 2
    assert M.sensor_moves([], [3, 1, 3]) == [(M.SENSOR_MOVE, 0), (M.SENSOR_MOVE, 1), (M.SENSOR_DISCARD, -1)]
    assert M.sensor_moves([4, 4], [4]) == [(M.SENSOR_MERGE, 0)]
