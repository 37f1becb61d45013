"""GPU tests: uzl_scanmerge_* against the NumPy restatement of its contract (tests/scanmerge_reference.py) on the scenes of
tests/scanmerge_scenes.py - merged ranges, intensities, the stage entry's bins and rho bit for bit, the scan centres equal - the
batch against single-pair calls, and the device-to-device hand-overs to the occupancy grid (with retired and renumbered scans)
and to the laser matcher against the same scans taken through the host."""
import contextlib

import numpy as np
import pytest

import scanmerge_reference as R
import scanmerge_scenes as S

pytestmark = pytest.mark.gpu

NAMES = sorted(S.scenes())


@pytest.fixture(scope="module")
def handle(capi):
    h = capi.ScanMerge()
    yield h
    h.close()


def _check_pair(h, pair, name):
    exp = S.expected(name)
    r, it, ce = h.read(pair)
    assert np.array_equal(r, exp["ranges"], equal_nan=True), name
    assert np.array_equal(it, exp["intensities"], equal_nan=True), name
    assert np.array_equal(ce, exp["center"]), name


@pytest.mark.parametrize("name", NAMES)
def test_one_pair_equals_the_restatement(handle, name):
    """beam counts 8, 63 / 64 / 65, 720, 4096 and n_a != n_b; empty bins and a finer b; NaN, +-inf and readings at, below and above
    each limit; cur at a.range_min / a.range_max; |cur - rho| on both sides of 0.1f; the negative x axis with y = +0 / -0; a point
    at the origin; identity displacements; b newer, older and equally old"""
    assert handle.run([S.scenes()[name]]) == 1
    exp = S.expected(name)
    for which in range(4):                                   # binning held apart from folding
        b, rho = handle.points(0, which)
        assert np.array_equal(b, exp["bin"][which]), (name, which)
        assert np.array_equal(rho, exp["rho"][which]), (name, which)
    _check_pair(handle, 0, name)


def test_no_pairs(handle, capi):
    assert handle.run([]) == 0
    with pytest.raises(capi.UzlError) as e:
        handle.read(0)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_300_pairs_equal_the_single_pair_calls(handle):
    """more workgroups than CUs, scenes of every size side by side: a pair's result does not depend on the others"""
    small = [n for n in NAMES if n != "n4096"]
    order = [small[(7 * i) % len(small)] for i in range(299)] + ["n4096"]
    assert handle.run([S.scenes()[n] for n in order]) == 300
    for i, name in enumerate(order):
        _check_pair(handle, i, name)
    for i in (0, 150, 299):
        b, rho = handle.points(i, R.DROP_RANGES)
        assert np.array_equal(b, S.expected(order[i])["bin"][R.DROP_RANGES]) and np.array_equal(rho, S.expected(order[i])["rho"][R.DROP_RANGES])
    # a run replaces the resident result
    assert handle.run([S.scenes()["n8"]]) == 1
    _check_pair(handle, 0, "n8")


GRID_NAMES = ["n720", "n65_b720", "finer_b_newer", "identity"]


def _poses(n):
    P = np.tile(np.eye(3, 4).reshape(12), (n, 1))
    P[:, 3] = 0.7 * np.arange(n)
    P[:, 7] = 0.3 * np.arange(n) % 1.1
    return P


def _grid_scan(name, node, ranges):
    a = S.scenes()[name][0]
    return dict(node=node, ranges=ranges, angle_min=float(a["angle_min"]), angle_increment=float(a["angle_increment"]), range_min=float(a["range_min"]))


def test_to_grid_equals_read_then_add_scans(handle, capi):
    handle.run([S.scenes()[n] for n in GRID_NAMES])
    P = _poses(len(GRID_NAMES))
    with contextlib.closing(capi.Grid()) as g1, contextlib.closing(capi.Grid()) as g2:
        assert handle.to_grid(g1, np.arange(len(GRID_NAMES))) == 0 and g1.scan_count() == len(GRID_NAMES)
        g2.add_scans([_grid_scan(n, i, handle.read(i)[0]) for i, n in enumerate(GRID_NAMES)])
        i1, i2 = g1.build(P), g2.build(P)
        assert i1 == i2 and i1["hits"] > 0
        assert np.array_equal(g1.read(), g2.read())
        for x, y in zip(g1.counts(), g2.counts()):
            assert np.array_equal(x, y)


def test_retired_and_renumbered_scans_equal_a_fresh_store(handle, capi):
    """nodes 0..3 each with a scan; 2 is merged into 1: their scans are retired, the merged one appended at node 1, the nodes behind
    the drop re-pointed - the build equals a fresh handle holding only the live scans at the compacted indices"""
    old = ["n720", "identity", "n65_b720", "n720_b65"]
    scans = [_grid_scan(n, i, S.scenes()[n][0]["ranges"]) for i, n in enumerate(old)]
    handle.run([S.scenes()["finer_b_older"]])
    merged = handle.read(0)[0]
    keep, drop = 1, 2
    old_to_new = np.array([0, 1, -1, 2], np.int32)
    P = _poses(3)
    with contextlib.closing(capi.Grid()) as g, contextlib.closing(capi.Grid()) as fresh:
        g.add_scans(scans)
        before = g.build(_poses(4))
        assert before["scans"] == 4
        first = handle.to_grid(g, [old_to_new[keep]])
        assert first == 4
        g.renumber_scans([0, 1, 2, 3], [old_to_new[0], -1, -1, old_to_new[3]])
        info = g.build(P)
        fresh.add_scans([dict(scans[0], node=0), dict(scans[3], node=2), _grid_scan("finer_b_older", 1, merged)])
        want = fresh.build(P)
        assert info == want and info["scans"] == 3
        assert np.array_equal(g.read(), fresh.read())
        for x, y in zip(g.counts(), fresh.counts()):
            assert np.array_equal(x, y)
        # an extend skips a retired scan too
        g.renumber_scans([4], [-1])
        assert g.extend(P, 0)["scans"] == 2


@pytest.mark.parametrize("use_near", [False, True])
def test_to_laser_equals_read_then_add_scans(handle, capi, use_near):
    names = ["n720", "identity", "n65_b720"]
    handle.run([S.scenes()[n] for n in names])
    with contextlib.closing(capi.Laser()) as l1, contextlib.closing(capi.Laser()) as l2:
        assert handle.to_laser(l1, use_near=use_near) == 0 and l1.scan_count() == 3
        scans = []
        for i, n in enumerate(names):
            a = S.scenes()[n][0]
            r, it, _ = handle.read(i)
            scans.append(dict(values=r if use_near else it, angle_min=float(a["angle_min"]), angle_increment=float(a["angle_increment"]),
                              range_min=float(a["range_min"]), range_max=float(a["range_max"])))
        l2.add_scans(scans)
        guess = S.planar(0.05, -0.03, 0.02)
        pairs = [(0, 1, guess), (1, 0, guess), (2, 2, np.eye(3, 4)), (0, 2, guess)]
        e1, e2 = l1.estimate(pairs), l2.estimate(pairs)
        assert e1.tobytes() == e2.tobytes()
