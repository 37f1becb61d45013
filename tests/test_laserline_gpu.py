"""GPU tests of uzl_laserline_* (laser line from depth images): ranges and intensities equal the NumPy restatement
tests/laserline_reference.py bit for bit and the scan centres exactly - the room scene through several camera transforms (the +-pi
seam included), both encodings, depth_scale, padded rows, odd image sizes, all-invalid and all-one-bin images, four angular grids,
groups of cameras, many images and several staging chunks in one call; results are deterministic and independent of how the images
were batched; to_grid equals read -> add_scans and the whole depth image -> map path equals NumPy; bad arguments change nothing."""
import ctypes as C
import math

import numpy as np
import pytest

import grid_reference as GR
import laserline_reference as LR
import laserline_scenes as LS

pytestmark = pytest.mark.gpu

F32 = np.float32
TRANSFORMS = {"level": LS.camera_transform(yaw=40.0), "pitched": LS.camera_transform(yaw=-75.0, pitch=20.0, height=0.9),
              "rolled": LS.camera_transform(yaw=130.0, roll=25.0, x=0.2, y=-0.1),
              "backwards": LS.camera_transform(yaw=180.0, pitch=5.0, height=0.5)}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    (r, i, c), (wr, wi, wc) = got, want
    assert r.shape == wr.shape and i.shape == wi.shape and c.shape == wc.shape
    assert np.array_equal(bits(r), bits(wr)), "ranges differ at %s" % (np.argwhere(bits(r) != bits(wr))[:5].tolist(),)
    assert np.array_equal(bits(i), bits(wi)), "intensities differ at %s" % (np.argwhere(bits(i) != bits(wi))[:5].tolist(),)
    assert np.array_equal(c, wc), "scan centres differ"


def check(capi, images, **cfg):
    h = capi.Laserline(**cfg)
    got = h.extract(images)
    h.close()
    want = LR.extract(images, **cfg)
    same(got, want)
    return want


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_room_through_camera_transforms(capi, u16):
    images = [LS.image(LS.room(seed=3 + k, u16=u16), T) for k, T in enumerate(TRANSFORMS.values())]
    r, i, c = check(capi, images)
    hi = F32(6)
    for k in range(len(images)):
        assert 100 < (r[k] < hi).sum() < 720 and (i[k] > 0).sum() >= (r[k] < hi).sum()      # each camera sees its part of the circle
    assert (r[3, :40] < hi).any() and (r[3, -40:] < hi).any()                                  # looking backwards: both sides of the seam
    assert np.abs(c[:, :2]).max() > 0.5 and (c[:, 2] == 0).all()


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_depth_scale_and_padded_rows(capi, u16):
    wide = np.zeros((120, 171), np.uint16 if u16 else F32)                  # rows 11 pixels wider than the image, step not a multiple of 16
    wide[:, :160] = LS.room(160, 120, seed=8, u16=u16)
    wide[:, 160:] = 1500 if u16 else 1.5                                    # never read
    images = [LS.image(wide[:, :160], TRANSFORMS["level"]), LS.image(LS.room(160, 120, seed=9, u16=u16), TRANSFORMS["backwards"])]
    check(capi, images, depth_scale=0.5)
    check(capi, images, depth_scale=1.0)
    arr, _ = capi.Laserline.pack_images(images)
    assert arr[0].step == 171 * wide.itemsize and arr[0].width == 160


def test_odd_sizes_and_degenerate_images(capi):
    T = TRANSFORMS["level"]
    one = np.full((1, 1), 2.0, F32)
    invalid = np.zeros((48, 64), F32); invalid[::2] = np.nan; invalid[1::4] = -1.0; invalid[3::4] = np.inf
    far = dict(LS.image(np.full((48, 64), 3.0, F32), LS.camera_transform(yaw=10.2, height=0.5)), fx=1e6, fy=1e6)   # every pixel in one bin
    images = [LS.image(one, T), LS.image(LS.room(3, 5, seed=1), T), LS.image(LS.room(5, 3, seed=1, u16=True), T),
              LS.image(LS.room(641, 479, seed=2), T), LS.image(LS.room(641, 479, seed=2, u16=True), TRANSFORMS["backwards"]),
              LS.image(invalid, T), LS.image(np.zeros((7, 9), np.uint16), T), far, LS.image(np.zeros((0, 0), F32), T)]
    r, i, c = check(capi, images)
    hi = F32(6)
    assert (r[0] < hi).sum() == 1 and (r[5] == hi).all() and (r[6] == hi).all() and (r[8] == hi).all() and (i[5] == 0).all()
    assert (r[7] < hi).sum() == 1 and c[5].tolist() == [0, 0, 0]


@pytest.mark.parametrize("inc", [math.pi / 360, 0.005, math.pi / 720, 6.2831855 / 4095.5], ids=["720", "1257", "1440", "4096"])
def test_angular_grids(capi, inc):
    assert LR.angular_grid(inc)[3] == {0: 720, 1: 1257, 2: 1440, 3: 4096}[[math.pi / 360, 0.005, math.pi / 720, 6.2831855 / 4095.5].index(inc)]
    images = [LS.image(LS.room(160, 120, seed=20 + k, u16=bool(k % 2)), T) for k, T in enumerate(TRANSFORMS.values())]
    r, _, _ = check(capi, images, angle_increment=inc)
    assert (r < F32(6)).sum() > 400
    r, i, c = check(capi, images, angle_increment=inc, min_height=5.0, max_height=6.0)         # heights that exclude everything
    assert (r == F32(6)).all() and (i == 0).all() and (c == 0).all()
    r, _, _ = check(capi, images, angle_increment=inc, min_height=-10.0, max_height=10.0, range_max=3.0, range_min=2.0)
    assert (r == F32(4)).any() and (r < F32(4)).any()


def rig(seed, n_nodes, cameras):
    """n_nodes nodes with cameras[node % len(cameras)] cameras each -> images with group = node.  The cameras of a node look 12
    degrees apart, so their scans overlap and the merge meets close and distant pairs."""
    rng = np.random.default_rng(seed)
    images = []
    for node in range(n_nodes):
        yaw = float(rng.uniform(-180, 180))
        for cam in range(cameras[node % len(cameras)]):
            T = LS.camera_transform(yaw=yaw + 12.0 * cam, pitch=float(rng.uniform(-5, 15)), height=float(rng.uniform(0.4, 0.8)))
            depth = LS.room(64, 48, seed=int(rng.integers(1 << 30)), lo=1.0, hi=5.5, u16=bool(rng.integers(2)))
            images.append(LS.image(depth, T, group=node))
    return images


def test_groups_of_cameras_and_batching(capi):
    images = rig(5, 130, (1, 2, 3))
    assert len(images) >= 250
    want = LR.extract(images)
    assert len(want[0]) == 130
    merged = want[0][1::3]                                      # the two-camera nodes: the merge made means and zeros
    assert (merged == 0).any()
    h = capi.Laserline()
    got = h.extract(images)
    same(got, want)
    same(h.extract(images), want)                               # a repeated call: identical
    same(h.read(), want)
    # the same nodes over several calls: whole groups per call, any split
    parts = []
    for a, b in ((0, 7), (7, 60), (60, 61), (61, 130)):
        parts.append(h.extract([im for im in images if a <= im["group"] < b]))
    same(tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), want)
    assert h.extract([])[0].shape == (0, 720)                   # no images: no scans
    h.close()


def test_300_images_in_one_call(capi):
    images = rig(6, 300, (1,))
    assert len(images) == 300
    check(capi, images)


def test_several_staging_chunks(capi):
    """120 images of 640 x 480 f32 (147 MB) go through the two staging halves in three chunks; four distinct images, repeated"""
    base = [LS.image(LS.room(seed=30 + k), T) for k, T in enumerate(TRANSFORMS.values())]
    want4 = LR.extract(base)
    images = [dict(base[k % 4], group=k) for k in range(120)]
    h = capi.Laserline()
    got = h.extract(images)
    same(got, tuple(np.concatenate([w] * 30) for w in want4))
    h.close()


def test_to_grid_equals_read_then_add_scans_and_the_reference(capi):
    n_nodes = 12
    images = rig(7, n_nodes, (2, 1))
    rng = np.random.default_rng(7)
    poses = np.zeros((n_nodes, 3, 4)); poses[:, :, :3] = np.eye(3)
    for k in range(n_nodes):
        poses[k, :, :3] = LS.rot("z", float(rng.uniform(-180, 180)))
        poses[k, :2, 3] = rng.uniform(-6, 6, 2)
    nodes = np.arange(n_nodes)[::-1].copy()                     # scan i belongs to node n - 1 - i
    cfg = dict(range_max=5.0)
    h = capi.Laserline()
    ranges, _, _ = h.extract(images)
    direct, via_host, ref = capi.Grid(**cfg), capi.Grid(**cfg), GR.GridReference(**cfg)
    pre = LR.grid_scans([np.full(90, 2.0, F32)], [3], angle_increment=math.pi / 45)           # a scan already in the store
    for g in (direct, via_host, ref):
        assert g.add_scans(pre) == 0
    assert h.to_grid(direct, nodes) == 1 and direct.scan_count() == 1 + n_nodes
    assert via_host.add_scans(LR.grid_scans(ranges, nodes)) == 1
    want_r, _, _ = LR.extract(images)
    ref.add_scans(LR.grid_scans(want_r, nodes))
    infos = [g.build(poses.reshape(-1, 12)) for g in (direct, via_host, ref)]
    for g in (direct, via_host):
        hits, passes = g.counts()
        rh, rp = ref.counts()
        assert np.array_equal(hits, rh) and np.array_equal(passes, rp) and np.array_equal(g.read(), ref.grid())
    assert infos[0] == infos[1] and infos[0]["hits"] == infos[2]["hits"] > 500 and infos[0]["scans"] == 1 + n_nodes
    assert h.to_grid(direct, nodes) == 1 + n_nodes              # again: appended behind
    # errors: nothing is appended
    count = direct.scan_count()
    L = capi.lib()
    assert L.uzl_laserline_to_grid(h._h, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_to_grid(h._h, direct._h, None, None) == capi.UZL_ERR_BAD_ARG
    bad = nodes.astype(np.int32); bad[3] = -1
    assert L.uzl_laserline_to_grid(h._h, direct._h, bad.ctypes.data_as(C.POINTER(C.c_int32)), None) == capi.UZL_ERR_BAD_ARG
    assert direct.scan_count() == count
    fresh = capi.Laserline()
    assert L.uzl_laserline_to_grid(fresh._h, direct._h, bad.ctypes.data_as(C.POINTER(C.c_int32)), None) == capi.UZL_ERR_STATE
    for x in (h, fresh, direct, via_host):
        x.close()


def test_bad_arguments_leave_the_result_as_it_was(capi):
    L = capi.lib()
    h = capi.Laserline()
    f32p = C.POINTER(C.c_float)
    assert L.uzl_laserline_read(h._h, 0, None, None, None) == capi.UZL_ERR_STATE              # nothing extracted yet
    images = rig(8, 5, (2,))
    want = LR.extract(images)
    same(h.extract(images), want)
    good = LS.image(LS.room(16, 12, seed=1), TRANSFORMS["level"], group=0)

    def refused(*ims, n=None, null=False):
        arr, keep = capi.Laserline.pack_images(list(ims))
        for im, a in zip(ims, arr):
            for k, v in im.get("raw", {}).items():
                setattr(a, k, v)
        rc = L.uzl_laserline_extract(h._h, C.c_int32(len(ims) if n is None else n), None if null else arr, None, None)
        assert rc == capi.UZL_ERR_BAD_ARG, (rc, ims[-1].get("raw"))
        assert L.uzl_laserline_last_error(h._h) != b""
        same(h.read(), want)

    refused(good, n=-1)
    refused(good, null=True)
    for raw in (dict(width=0), dict(height=0), dict(width=-1), dict(data=None), dict(step=16 * 4 - 1), dict(encoding=2), dict(encoding=-1)):
        refused(dict(good, raw=raw))
    for k in ("fx", "fy"):
        for v in (0.0, math.nan, math.inf):
            refused(dict(good, **{k: v}))
    for k in ("cx", "cy"):
        for v in (math.nan, -math.inf):
            refused(dict(good, **{k: v}))
    T = np.array(good["camera_transform"]); T[1, 2] = math.nan
    refused(dict(good, camera_transform=T))
    refused(good, dict(good, group=2))                          # a gap
    refused(dict(good, group=1), good)                          # descending
    refused(good, dict(good, group=1), dict(good, group=0))     # not contiguous
    empty_with_data = dict(good, raw=dict(width=0, height=0))
    refused(empty_with_data)
    # read: truncated and partial outputs
    r = np.zeros((5, 720), F32)
    assert L.uzl_laserline_read(h._h, 4, r.ctypes.data_as(f32p), None, None) == -9
    assert L.uzl_laserline_read(h._h, -1, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_read(h._h, 9, r.ctypes.data_as(f32p), None, None) == 5 and np.array_equal(bits(r), bits(want[0]))
    # set_config: checked like create, the device cannot change, the resident scans keep their grid
    with pytest.raises(capi.UzlError):
        h.set_config(angle_increment=3.0)
    h.cfg.angle_increment = math.pi / 360
    with pytest.raises(capi.UzlError):
        h.set_config(device=1 + capi.device_count())
    h.cfg.device = 0
    h.set_config(angle_increment=0.005, range_max=4.0)
    same(h.read(), want)
    same(h.extract(images), LR.extract(images, angle_increment=0.005, range_max=4.0))
    h.close()
