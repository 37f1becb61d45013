"""GPU tests of uzl_grid_* (occupancy-grid projection): counts, classified cells and totals equal the NumPy restatement
tests/grid_reference.py exactly on ray-cast room scenes (NaN / inf beams, two scans on some nodes, absent nodes, a sensor outside
the grid, range_max > max_distance), at the deployed point with 2,000 nodes, and by closed-form sums at 20,000; extend equals the
restatement's extend; builds are deterministic and independent of how the scans were batched; bad arguments change nothing."""
import ctypes as C
import math

import numpy as np
import pytest

import grid_reference as GR
import grid_scenes as GS

pytestmark = pytest.mark.gpu


def same(g, r, info=None, rinfo=None):
    h, p = g.counts()
    rh, rp = r.counts()
    assert np.array_equal(h, rh) and np.array_equal(p, rp)
    assert np.array_equal(g.read(), r.grid())
    if info is not None:
        for k in ("width", "height", "valid_beams", "hits", "scans", "off_grid"):
            assert info[k] == rinfo[k], (k, info[k], rinfo[k])
        for k in ("origin_x", "origin_y", "resolution"):
            assert info[k] == rinfo[k], k


def mixed_scene(n, seed, cfg):
    rng = np.random.default_rng(seed)
    poses, scans = GS.scene(n, seed=seed, n_beams=360, angle_increment=math.pi / 180, scan_range_max=cfg.get("range_max", 5.0))
    GS.sprinkle(scans, rng)
    extra = []
    for s in scans[::7]:                                                       # a second scan on every 7th node, another sensor
        D = np.eye(3, 4); D[:2, :2] = [[0, -1], [1, 0]]; D[:, 3] = [-0.05, 0.1, 0.2]
        extra.append(dict(s, ranges=s["ranges"][::-1].copy(), displacement=D.reshape(12)))
    far = np.eye(3, 4); far[0, 3] = 1e3                                         # a sensor far outside the grid
    extra.append(dict(scans[3], displacement=far.reshape(12)))
    near = np.eye(3, 4); near[1, 3] = -(5 * cfg.get("range_max", 5.0) + 3.0)     # just outside the border, rays reach in
    extra.append(dict(scans[5], displacement=near.reshape(12)))
    extra.append(dict(scans[0], node=n + 5))                                   # a node past n_nodes
    extra.append(dict(scans[1], ranges=np.zeros(0, np.float32)))               # no beams
    r = scans[2]["ranges"].copy(); r[:5] = [np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0)), 0.0, 1e9, -1.0]
    extra.append(dict(scans[2], ranges=r))
    present = (rng.random(n) > 0.1).astype(np.uint8)
    present[0] = 1
    return poses, scans + extra, present


CFGS = [dict(), dict(range_max=5.0, resolution=0.05), dict(range_max=8.0, max_distance=3.0, resolution=0.07, min_pass_through=2),
        dict(range_max=4.0, occupancy_threshold=0.3, known_free_radius=1.3, resolution=0.13)]


@pytest.mark.parametrize("ci", range(len(CFGS)))
def test_mixed_scene_equals_the_reference(capi, ci):
    cfg = CFGS[ci]
    poses, scans, present = mixed_scene(150, ci, cfg)
    g = capi.Grid(**cfg)
    r = GR.GridReference(**cfg)
    assert g.add_scans(scans) == 0 and r.add_scans(scans) == 0
    info, rinfo = g.build(poses, present), r.build(poses, present)
    same(g, r, info, rinfo)
    assert info["hits"] == int(g.counts()[0].sum())
    info, rinfo = g.build(poses), r.build(poses)                              # all present: another geometry, rebuilt from zero
    same(g, r, info, rinfo)
    g.close()


def test_deployed_point_2000_nodes(capi):
    cfg = dict(range_max=GS.DEPLOYED["range_max"], resolution=GS.DEPLOYED["resolution"])
    poses, scans = GS.scene(2000, seed=11)
    GS.sprinkle(scans, np.random.default_rng(11), frac=0.005)
    g, r = capi.Grid(**cfg), GR.GridReference(**cfg)
    g.add_scans(scans); r.add_scans(scans)
    info, rinfo = g.build(poses), r.build(poses)
    same(g, r, info, rinfo)
    assert (g.read() == 100).sum() > 1000 and (g.read() == 0).sum() > 100000
    g.close()


def test_20k_nodes_closed_form(capi):
    cfg = dict(range_max=GS.DEPLOYED["range_max"], resolution=GS.DEPLOYED["resolution"])
    poses, scans = GS.scene(20000, seed=12)
    g = capi.Grid(**cfg)
    g.add_scans(scans)
    info = g.build(poses)
    h, p = g.counts()
    ox, oy, res = info["origin_x"], info["origin_y"], info["resolution"]
    W, H = info["width"], info["height"]
    full = dict(GR.DEFAULTS, **cfg)
    n_hit = n_valid = steps = 0
    for s in scans:
        S = GR.compose(poses[s["node"]], s["displacement"])
        v, ex, ey, hit = GR.beams(full, s, S)
        cx, cy = GR.cell(ex, ox, res), GR.cell(ey, oy, res)
        if len(cx):
            assert cx.min() >= 0 and cy.min() >= 0 and cx.max() < W and cy.max() < H    # every cell in bounds
        ocx, ocy = int(GR.cell(S[3], ox, res)), int(GR.cell(S[7], oy, res))
        n_valid += v
        n_hit += int(hit.sum())
        steps += int((np.maximum(np.abs(cx - ocx), np.abs(cy - ocy)) + 1).sum())
    k = int(full["known_free_radius"] / res)
    free = np.zeros((H, W), bool)
    for i in range(len(poses)):
        x, y = int(GR.cell(poses[i, 3], ox, res)), int(GR.cell(poses[i, 7], oy, res))
        free[max(y - k, 0):y + k + 1, max(x - k, 0):x + k + 1] = True
    assert info["valid_beams"] == n_valid and info["hits"] == n_hit
    assert int(h.sum(dtype=np.int64)) == n_hit
    assert int(p.sum(dtype=np.int64)) == steps + full["min_pass_through"] * int(free.sum())
    g.close()


@pytest.mark.parametrize("k,seed", [(60, 3), (140, 4)])
def test_extend_equals_the_reference(capi, k, seed):
    cfg = dict(range_max=3.0, resolution=0.05)
    poses, scans, present = mixed_scene(200, seed, cfg)
    g, r = capi.Grid(**cfg), GR.GridReference(**cfg)
    g.add_scans(scans); r.add_scans(scans)
    same(g, r, g.build(poses[:k], present[:k]), r.build(poses[:k], present[:k]))
    info, rinfo = g.extend(poses, k, present), r.extend(poses, k, present)
    same(g, r, info, rinfo)
    assert info["off_grid"] == rinfo["off_grid"] == 0                          # 200 nodes stay well inside the 15 m margin
    i0 = g.info()
    moved = poses.copy()                                                       # the last ten nodes within range_max of the border
    moved[190:, 3] = i0["origin_x"] + i0["width"] * i0["resolution"] - 1.0 - 0.1 * np.arange(10)
    info, rinfo = g.extend(moved, 190), r.extend(moved, 190)
    same(g, r, info, rinfo)
    assert info["off_grid"] == rinfo["off_grid"] == 1
    g.close()


def test_deterministic_and_batch_independent(capi):
    cfg = dict(range_max=5.0, resolution=0.05)
    poses, scans, present = mixed_scene(300, 7, cfg)
    a, b = capi.Grid(**cfg), capi.Grid(**cfg)
    a.add_scans(scans)
    for i in range(0, len(scans), 13):
        b.add_scans(scans[i:i + 13])
    assert a.scan_count() == b.scan_count() == len(scans)
    ia = a.build(poses, present)
    first = (a.counts(), a.read())
    assert a.build(poses, present) == ia and b.build(poses, present) == ia
    for g in (a, b):
        (h, p), grid = g.counts(), g.read()
        assert np.array_equal(h, first[0][0]) and np.array_equal(p, first[0][1]) and np.array_equal(grid, first[1])
    a.close(); b.close()


def test_bad_arguments_change_nothing(capi):
    cfg = dict(range_max=3.0, resolution=0.1)
    poses, scans, _ = mixed_scene(40, 9, cfg)
    g = capi.Grid(**cfg)
    L = capi.lib()
    with pytest.raises(capi.UzlError) as e:
        g.extend(poses, 0)
    assert e.value.status == capi.UZL_ERR_STATE
    g.add_scans(scans)
    info = g.build(poses)
    before = (g.counts(), g.read(), g.scan_count(), info)

    def unchanged():
        (h, p), grid = g.counts(), g.read()
        assert np.array_equal(h, before[0][0]) and np.array_equal(p, before[0][1]) and np.array_equal(grid, before[1])
        assert g.scan_count() == before[2] and g.info() == before[3]

    def code(fn, *a):
        with pytest.raises(capi.UzlError) as e:
            fn(*a)
        return e.value.status

    bad_scans = [dict(scans[0], node=-1), dict(scans[0], angle_increment=np.float32(np.inf)),
                 dict(scans[0], angle_min=np.float32(np.nan)), dict(scans[0], range_min=np.float32(-0.1)),
                 dict(scans[0], range_min=np.float32(np.nan)), dict(scans[0], displacement=np.full(12, np.nan))]
    for s in bad_scans:
        assert code(g.add_scans, [scans[1], s]) == capi.UZL_ERR_BAD_ARG
        unchanged()
    arr, keep = g.pack_scans([scans[0]])
    arr[0].n_ranges = -1
    assert L.uzl_grid_add_scans(g._h, 1, arr, None) == capi.UZL_ERR_BAD_ARG
    arr[0].n_ranges = 5; arr[0].ranges = None
    assert L.uzl_grid_add_scans(g._h, 1, arr, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_grid_add_scans(g._h, -1, arr, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_grid_add_scans(g._h, 1, None, None) == capi.UZL_ERR_BAD_ARG
    unchanged()
    P = poses.copy(); P[3, 0] = np.nan
    assert code(g.build, P) == capi.UZL_ERR_BAD_ARG
    assert code(g.extend, P, 0) == capi.UZL_ERR_BAD_ARG
    pr = np.ones(len(poses), np.uint8); pr[3] = 0
    g2info = g.build(P, pr)                                                    # a non-finite pose of an absent node is fine
    assert g2info["scans"] < info["scans"]
    g.build(poses)
    unchanged()
    assert code(g.build, poses, np.zeros(len(poses), np.uint8)) == capi.UZL_ERR_BAD_ARG   # no present node
    assert code(g.extend, poses, -1) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_grid_build(g._h, -1, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_grid_build(g._h, 3, None, None, None) == capi.UZL_ERR_BAD_ARG
    far = poses.copy(); far[0, 3] = 1e7                                         # width * height beyond max_cells
    assert code(g.build, far) == capi.UZL_ERR_BAD_ARG
    huge = poses.copy(); huge[5, :3] *= 1e9                                     # rays scaled beyond 2^24 cells
    assert code(g.build, huge) == capi.UZL_ERR_BAD_ARG
    out = np.zeros(5, np.int8)
    assert L.uzl_grid_read(g._h, C.c_int64(5), out.ctypes.data_as(C.POINTER(C.c_int8))) == -9
    assert L.uzl_grid_counts(g._h, C.c_int64(5), None, None) == -9
    unchanged()
    bad_cfg = capi.GridCfg.from_buffer_copy(g.cfg); bad_cfg.resolution = 0.0
    assert L.uzl_grid_set_config(g._h, C.byref(bad_cfg)) == capi.UZL_ERR_BAD_ARG
    unchanged()
    g.close()


def test_new_config_takes_effect_at_the_next_full_build(capi):
    poses, scans, _ = mixed_scene(60, 10, dict(range_max=3.0))
    g, r = capi.Grid(range_max=3.0), GR.GridReference(range_max=3.0)
    g.add_scans(scans); r.add_scans(scans)
    g.build(poses[:30]); r.build(poses[:30])
    g.set_config(resolution=0.05)
    r.cfg["resolution"] = 0.05
    same(g, r, g.extend(poses, 30), r.extend(poses, 30))                       # extend keeps the build's 0.1
    assert g.info()["resolution"] == 0.1
    same(g, r, g.build(poses), r.build(poses))
    assert g.info()["resolution"] == 0.05
    g.close()
