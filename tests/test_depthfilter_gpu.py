"""GPU tests of uzl_depthfilter_* (depth refinement and 3-D keypoint lifting): the refined images equal the NumPy restatement
tests/depthfilter_reference.py bit for bit - images smaller than the halo, one pixel either side of the tile, VGA in both
encodings, padded rows, depth_scale, invalid pixels, the ends of the colour table, the ends of both radii, the filter off, empty
images; results do not depend on batching and repeat; the lift equals the restatement bit for bit; to_laserline equals read ->
uzl_laserline_extract and the whole depth image -> map path equals NumPy; the lifted arrays go into the estimator; bad arguments
change nothing."""
import ctypes as C
import math

import numpy as np
import pytest

import depthfilter_reference as DR
import depthfilter_scenes as DS
import grid_reference as GR
import laserline_reference as LR
import laserline_scenes as LS

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE_W, TILE_H = 64, 32                     # depthfilter_types.hpp: kDepthTileW, kDepthTileH


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_image(got, want, what=""):
    assert got.shape == want.shape and got.dtype == F32, (what, got.shape, want.shape)
    diff = np.argwhere(bits(got) != bits(want))
    assert len(diff) == 0, "%s: %d pixels differ, first at %s" % (what, len(diff), diff[:5].tolist())


def check(capi, scenes, **cfg):
    """refine the (image, guide) pairs in one call and compare every image with the restatement -> the refined images"""
    h = capi.DepthFilter(**cfg)
    guides = None if all(g is None for _, g in scenes) else [g for _, g in scenes]
    h.refine([im for im, _ in scenes], guides)
    assert h.image_count() == len(scenes)
    out = []
    for k, (im, g) in enumerate(scenes):
        got = h.read(k)
        same_image(got, DR.refine(im["depth"], g, **cfg), "image %d %s %s" % (k, im["depth"].shape, cfg))
        out.append(got)
    h.close()
    return out


def test_images_smaller_than_the_halo(capi):
    scenes = [DS.scene(w, h, seed=w, u16=u16, kind="noise") for (w, h), u16 in (((1, 1), False), ((3, 5), False), ((5, 3), True), ((7, 9), False),
                                                                               ((1, 6), True), ((6, 1), False), ((2, 2), False))]
    out = check(capi, scenes)
    assert any((o != 0).any() for o in out)


def test_one_pixel_either_side_of_the_tile(capi):
    sizes = [(TILE_W + dx, TILE_H + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)] + [(2 * TILE_W + 1, 2 * TILE_H + 1)]
    out = check(capi, [DS.scene(w, h, seed=10 + k, u16=bool(k % 2)) for k, (w, h) in enumerate(sizes)])
    assert all((o != 0).mean() > 0.5 for o in out)


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_vga_plus_one_minus_one(capi, u16):
    (out,) = check(capi, [DS.scene(641, 479, seed=2, u16=u16)])
    assert (out != 0).mean() > 0.6 and len(np.unique(out)) > 1000


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_padded_rows_and_depth_scale(capi, u16):
    wide = np.zeros((60, 171), np.uint16 if u16 else F32)                   # rows 11 pixels wider than the image, step not a multiple of 16
    wide[:, :160] = DS.depth(160, 60, seed=8, u16=u16)
    wide[:, 160:] = 1500 if u16 else 1.5                                    # never read
    gwide = np.full((60, 173), 77, np.uint8)
    gwide[:, :160] = DS.guide(160, 60, seed=8)
    scene = (LS.image(wide[:, :160]), gwide[:, :160])
    arr, _ = capi.Laserline.pack_images([scene[0]])
    garr, _ = capi.DepthFilter.pack_guides([scene[1]])
    assert arr[0].step == 171 * wide.itemsize and garr[0].step == 173 and garr[0].width == 160
    a, = check(capi, [scene])
    b, = check(capi, [scene], depth_scale=0.5)
    same_image(a, check(capi, [(LS.image(np.ascontiguousarray(wide[:, :160])), np.ascontiguousarray(gwide[:, :160]))])[0])
    assert not np.array_equal(a, b)


def test_invalid_pixels(capi):
    invalid = np.zeros((48, 64), F32); invalid[::2] = np.nan; invalid[1::4] = -1.0; invalid[3::4] = np.inf
    mixed = DS.depth(80, 50, seed=5); mixed[10] = np.nan; mixed[20] = np.inf; mixed[30] = -1.0; mixed[40, ::3] = -np.inf
    g = DS.guide(64, 48, seed=5)
    out = check(capi, [(LS.image(np.zeros((48, 64), F32)), g), (LS.image(np.zeros((48, 64), np.uint16)), g), (LS.image(invalid), g),
                       (LS.image(mixed), DS.guide(80, 50, seed=6))])
    assert not out[0].any() and not out[1].any() and not out[2].any()       # NaN rows poison every window
    assert not out[3][7:14].any() and not out[3][17:24].any() and not out[3][37:44].any() and out[3][:7].any()
    assert np.isfinite(out[3]).all()


def test_the_ends_of_the_colour_table(capi):
    im, _ = DS.scene(90, 40, seed=7)
    extremes = DS.guide(90, 40, kind="extremes")
    assert int(extremes.max()) - int(extremes.min()) == 255                 # table index 255
    a, b, c = check(capi, [(im, extremes), (im, DS.guide(90, 40, kind="flat")), (im, DS.guide(90, 40, seed=7, kind="noise"))])
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
    check(capi, [(im, extremes), (im, DS.guide(90, 40, seed=7))], sigma_color=300.0, sigma_space=0.0)


@pytest.mark.parametrize("cfg", [dict(radius=0), dict(nearest_radius=0), dict(radius=0, nearest_radius=0), dict(radius=1, nearest_radius=7),
                                 dict(radius=15, nearest_radius=7), dict(radius=15, nearest_radius=0)],
                         ids=["R0", "P0", "R0P0", "R1P7", "R15P7", "R15P0"])
def test_the_ends_of_both_radii(capi, cfg):
    check(capi, [DS.scene(TILE_W + 3, TILE_H + 2, seed=11, nans=0.0), DS.scene(5, 4, seed=12, u16=True), DS.scene(16, 70, seed=13)], **cfg)


def test_the_filter_off_and_empty_images(capi):
    scenes = [DS.scene(70, 33, seed=14), DS.scene(9, 7, seed=15, u16=True), (LS.image(LS.room(40, 20, seed=16)), None)]
    a = check(capi, [(im, None) for im, _ in scenes], use_bilateral_filter=0)
    assert np.isnan(a[2]).any() and np.array_equal(bits(a[2]), bits(scenes[2][0]["depth"]))
    check(capi, [(im, None) for im, _ in scenes[:2]], use_bilateral_filter=0, depth_scale=0.5)
    empty = (LS.image(np.zeros((0, 0), F32)), np.zeros((0, 0), np.uint8))
    out = check(capi, [empty, scenes[0], empty])
    assert out[0].shape == (0, 0) and out[1].shape == (33, 70)
    h = capi.DepthFilter()
    h.refine([], [])                                                        # no images: an empty set
    assert h.image_count() == 0
    h.close()


def test_batching_changes_nothing_and_calls_repeat(capi):
    sizes = [(70, 40), (1, 1), (129, 65), (64, 32), (33, 130), (5, 3), (200, 17), (63, 31), (0, 0)]
    scenes = [DS.scene(w, h, seed=20 + k, u16=bool(k % 3 == 1)) for k, (w, h) in enumerate(sizes)]
    h = capi.DepthFilter()
    h.refine([im for im, _ in scenes], [g for _, g in scenes])
    together = [h.read(k) for k in range(9)]
    h.refine([im for im, _ in scenes], [g for _, g in scenes])
    for k in range(9):
        same_image(h.read(k), together[k], "second call, image %d" % k)
    for k, (im, g) in enumerate(scenes):
        h.refine([im], [g])
        assert h.image_count() == 1
        same_image(h.read(0), together[k], "alone, image %d" % k)
        same_image(together[k], DR.refine(im["depth"], g), "restatement, image %d" % k)
    h.close()


def test_the_lift_equals_the_restatement(capi):
    (im, g), (im2, _) = DS.scene(66, 34, seed=30), DS.scene(40, 20, seed=31)
    im = dict(im, fy=1.1 * im["fx"], cy=im["cy"] + 0.25)
    rng = np.random.default_rng(30)
    u = rng.integers(-6, 72, 700).astype(np.int32); v = rng.integers(-6, 40, 700).astype(np.int32)
    h = capi.DepthFilter()
    h.refine([im, im2], [g, DS.guide(40, 20, seed=31)])
    image = h.read(0)
    zero_v, zero_u = np.argwhere(image == 0)[:5].T                          # keypoints on invalid (0) pixels
    u = np.concatenate([u, zero_u.astype(np.int32)]); v = np.concatenate([v, zero_v.astype(np.int32)])
    median = float(np.median(image[image > 0]))
    for max_depth in (0.0, median, 0.5, 100.0):
        pos, valid = h.lift(0, u, v, max_depth)
        wpos, wvalid = DR.lift(image, u, v, im["fx"], im["fy"], im["cx"], im["cy"], max_depth)
        assert pos.dtype == np.float64 and np.array_equal(np.ascontiguousarray(pos).view(np.uint64), np.ascontiguousarray(wpos).view(np.uint64))
        assert np.array_equal(valid, wvalid) and not valid[-5:].any()
    assert 0 < h.lift(0, u, v, median)[1].sum() < h.lift(0, u, v, 0.0)[1].sum() and not h.lift(0, u, v, 0.5)[1].any()
    pos, valid = h.lift(1, [3, 39, 40], [2, 19, -1])                        # the second image, its own intrinsics
    wpos, wvalid = DR.lift(h.read(1), [3, 39, 40], [2, 19, -1], im2["fx"], im2["fy"], im2["cx"], im2["cy"])
    assert np.array_equal(pos, wpos) and np.array_equal(valid, wvalid)
    pos, valid = h.lift(0, [], [])
    assert pos.shape == (3, 0) and valid.shape == (0,)
    # the filter off: NaN and infinite pixels stay in the image; a keypoint on NaN is invalid, one on +inf lifts to infinities
    raw = LS.room(40, 20, seed=32); raw[4, 5] = np.nan; raw[6, 7] = np.inf; raw[8, 9] = 0.0
    h.set_config(use_bilateral_filter=0)
    h.refine([LS.image(raw)])
    pos, valid = h.lift(0, [5, 7, 9, 11], [4, 6, 8, 10])
    wpos, wvalid = DR.lift(raw, [5, 7, 9, 11], [4, 6, 8, 10], *[LS.image(raw)[k] for k in ("fx", "fy", "cx", "cy")])
    assert valid.tolist() == wvalid.tolist() == [0, 1, 0, int(raw[10, 11] != 0 and not np.isnan(raw[10, 11]))]
    assert np.array_equal(pos.view(np.uint64), wpos.view(np.uint64)) and np.isinf(pos[:, 1]).all()
    h.close()


TRANSFORMS = [LS.camera_transform(yaw=40.0), LS.camera_transform(yaw=52.0, pitch=10.0, height=0.7),
              LS.camera_transform(yaw=180.0, pitch=5.0, height=0.5), LS.camera_transform(yaw=-75.0, pitch=20.0, height=0.9)]


def rig():
    """two nodes of two cameras each (groups 0, 0, 1, 1), the third image looking backwards across the +-pi seam; widths that are
    and are not a multiple of 4 (the bin kernel's vector loads)"""
    sizes = [(160, 120), (161, 90), (160, 120), (66, 50)]
    return [DS.scene(w, h, seed=40 + k, u16=bool(k == 1), T=T, group=k // 2, lo=1.0, hi=5.5) for k, ((w, h), T) in enumerate(zip(sizes, TRANSFORMS))]


def same_scans(got, want):
    for a, b, name in zip(got, want, ("ranges", "intensities", "centres")):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8 if a.dtype != F32 else np.uint32), b.view(np.uint8 if b.dtype != F32 else np.uint32)), name


def test_to_laserline_equals_read_then_extract(capi):
    scenes = rig()
    h, direct, via_host = capi.DepthFilter(), capi.Laserline(), capi.Laserline()
    L = capi.lib()
    assert L.uzl_depthfilter_to_laserline(h._h, direct._h, None, None) == capi.UZL_ERR_STATE          # no refine yet
    h.refine([im for im, _ in scenes], [g for _, g in scenes])
    got = h.to_laserline(direct)
    refined = [dict(im, depth=h.read(k)) for k, (im, _) in enumerate(scenes)]
    want = via_host.extract(refined)
    same_scans(got, want)
    assert got[0].shape == (2, 720)
    hi = F32(6)
    assert (got[0][1, :40] < hi).any() and (got[0][1, -40:] < hi).any()     # the backwards camera: both sides of the seam
    same_scans(got, LR.extract([dict(im, depth=DR.refine(im["depth"], g)) for im, g in scenes]))
    same_scans(h.to_laserline(direct), want)                                # again: identical, the set is still resident
    same_scans(direct.read(), want)
    # other angular grid and heights: the laser-line handle's own config applies
    direct.set_config(angle_increment=0.005, min_height=-1.0, max_height=2.0)
    via_host.set_config(angle_increment=0.005, min_height=-1.0, max_height=2.0)
    same_scans(h.to_laserline(direct), via_host.extract(refined))
    # refused: a laser-line handle that would scale again, a NULL handle; its resident scans stay
    kept = direct.read()
    direct.set_config(depth_scale=0.5)
    assert L.uzl_depthfilter_to_laserline(h._h, direct._h, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_last_error(h._h) != b"" and L.uzl_laserline_last_error(direct._h) != b""
    assert L.uzl_depthfilter_to_laserline(h._h, None, None, None) == capi.UZL_ERR_BAD_ARG
    same_scans(direct.read(), kept)
    # an empty set gives no scans
    direct.set_config(depth_scale=1.0)
    h.refine([], [])
    assert h.to_laserline(direct)[0].shape == (0, 1257)
    for x in (h, direct, via_host):
        x.close()


def test_depth_image_to_map_equals_numpy(capi):
    scenes = rig()
    nodes = np.array([1, 0])
    poses = np.zeros((2, 3, 4)); poses[:, :, :3] = np.eye(3)
    poses[1, :, :3] = LS.rot("z", 30.0); poses[1, :2, 3] = [1.5, -0.5]
    h, line = capi.DepthFilter(), capi.Laserline()
    h.refine([im for im, _ in scenes], [g for _, g in scenes])
    h.to_laserline(line)
    cfg = dict(range_max=5.0)
    grid, ref = capi.Grid(**cfg), GR.GridReference(**cfg)
    assert line.to_grid(grid, nodes) == 0
    want_r, _, _ = LR.extract([dict(im, depth=DR.refine(im["depth"], g)) for im, g in scenes])
    ref.add_scans(LR.grid_scans(want_r, nodes))
    info, rinfo = grid.build(poses.reshape(-1, 12)), ref.build(poses.reshape(-1, 12))
    hits, passes = grid.counts()
    rh, rp = ref.counts()
    assert np.array_equal(hits, rh) and np.array_equal(passes, rp) and np.array_equal(grid.read(), ref.grid())
    assert info["hits"] == rinfo["hits"] > 100 and info["scans"] == 2
    for x in (h, line, grid):
        x.close()


def test_the_lifted_arrays_go_into_the_estimator(capi):
    im, g = DS.scene(160, 120, seed=50)
    h = capi.DepthFilter()
    h.refine([im], [g])
    rng = np.random.default_rng(50)
    n = 300
    u, v = rng.integers(0, 160, n).astype(np.int32), rng.integers(0, 120, n).astype(np.int32)
    pos, valid = h.lift(0, u, v, 10.0)
    assert pos.shape == (3, n) and 0 < valid.sum() < n
    m = capi.Match()
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    a, b = m.add_frame(desc, pos, valid), m.add_frame(desc, pos, valid)
    assert a >= 0 and b == a + 1
    m.close()
    h.close()


def test_bad_arguments_leave_the_resident_set_as_it_was(capi):
    L = capi.lib()
    h = capi.DepthFilter()
    f32p, i32p, f64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    assert L.uzl_depthfilter_image_count(h._h) == capi.UZL_ERR_STATE        # nothing refined yet
    assert L.uzl_depthfilter_read(h._h, 0, None, C.c_int64(0)) == capi.UZL_ERR_STATE
    assert L.uzl_depthfilter_lift(h._h, 0, 0, None, None, C.c_double(0.0), None, None) == capi.UZL_ERR_STATE
    scenes = [DS.scene(70, 40, seed=60), DS.scene(20, 12, seed=61, u16=True)]
    h.refine([im for im, _ in scenes], [g for _, g in scenes])
    want = [DR.refine(im["depth"], g) for im, g in scenes]

    def unchanged():
        assert h.image_count() == 2
        for k in range(2):
            same_image(h.read(k), want[k])

    good, gg = DS.scene(16, 12, seed=1)

    def refused(ims, guides, n=None, null=False, null_guides=False, raw=None, graw=None):
        arr, keep = capi.Laserline.pack_images(ims)
        garr, gkeep = capi.DepthFilter.pack_guides(guides)
        for k, val in (raw or {}).items():
            setattr(arr[len(ims) - 1], k, val)
        for k, val in (graw or {}).items():
            setattr(garr[len(ims) - 1], k, val)
        rc = L.uzl_depthfilter_refine(h._h, C.c_int32(len(ims) if n is None else n), None if null else arr, None if null_guides else garr)
        assert rc == capi.UZL_ERR_BAD_ARG, (rc, raw, graw)
        assert L.uzl_depthfilter_last_error(h._h) != b""
        unchanged()

    refused([good], [gg], n=-1)
    refused([good], [gg], null=True)
    refused([good], [gg], null_guides=True)
    for raw in (dict(width=0), dict(height=0), dict(width=-1), dict(data=None), dict(step=16 * 4 - 1), dict(encoding=2)):
        refused([good], [gg], raw=raw)
    for graw in (dict(width=15), dict(height=13), dict(data=None), dict(step=15), dict(width=0, height=0)):
        refused([good], [gg], graw=graw)
    refused([good], [DS.guide(12, 16)])                                     # transposed
    for k, val in (("fx", 0.0), ("fy", math.nan), ("cx", math.inf), ("cy", math.nan)):
        refused([dict(good, **{k: val})], [gg])
    T = np.array(good["camera_transform"]); T[1, 2] = math.nan
    refused([dict(good, camera_transform=T)], [gg])
    refused([dict(good, group=0), dict(good, group=2)], [gg, gg])           # a gap in the groups
    # read and lift
    out = np.zeros(70 * 40, F32)
    assert L.uzl_depthfilter_read(h._h, 0, None, C.c_int64(0)) == 70 * 40    # the size
    assert L.uzl_depthfilter_read(h._h, 0, out.ctypes.data_as(f32p), C.c_int64(70 * 40 - 1)) == -9
    assert L.uzl_depthfilter_read(h._h, 0, out.ctypes.data_as(f32p), C.c_int64(-1)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_read(h._h, 2, out.ctypes.data_as(f32p), C.c_int64(out.size)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_read(h._h, -1, out.ctypes.data_as(f32p), C.c_int64(out.size)) == capi.UZL_ERR_BAD_ARG
    u = np.zeros(4, np.int32); pos = np.zeros(12); valid = np.zeros(4, np.uint8)
    args = (u.ctypes.data_as(i32p), u.ctypes.data_as(i32p))
    outs = (pos.ctypes.data_as(f64p), valid.ctypes.data_as(u8p))
    assert L.uzl_depthfilter_lift(h._h, 0, 4, *args, C.c_double(0.0), *outs) == capi.UZL_OK
    assert L.uzl_depthfilter_lift(h._h, 2, 4, *args, C.c_double(0.0), *outs) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(h._h, 0, -1, *args, C.c_double(0.0), *outs) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(h._h, 0, 4, None, args[1], C.c_double(0.0), *outs) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(h._h, 0, 4, *args, C.c_double(0.0), None, outs[1]) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(h._h, 0, 4, *args, C.c_double(math.nan), *outs) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(h._h, 0, 4, *args, C.c_double(-1.0), *outs) == capi.UZL_ERR_BAD_ARG
    unchanged()
    # set_config: checked like create, the device cannot change, the resident images stay
    with pytest.raises(capi.UzlError):
        h.set_config(radius=16)
    h.cfg.radius = 3
    with pytest.raises(capi.UzlError):
        h.set_config(device=1 + capi.device_count())
    h.cfg.device = 0
    h.set_config(radius=2, sigma_color=20.0)
    unchanged()
    h.refine([im for im, _ in scenes], [g for _, g in scenes])
    same_image(h.read(0), DR.refine(scenes[0][0]["depth"], scenes[0][1], radius=2, sigma_color=20.0))
    # a 0 x 0 image has no pixel to lift from
    h.refine([LS.image(np.zeros((0, 0), F32))], [np.zeros((0, 0), np.uint8)])
    assert L.uzl_depthfilter_lift(h._h, 0, 4, *args, C.c_double(0.0), *outs) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(h._h, 0, 0, None, None, C.c_double(0.0), None, None) == capi.UZL_OK
    h.close()


def test_three_staging_chunks_by_the_image_count(capi):
    """2 * 8192 + 5 small images cross the stager's image-count limit (image_stager.hpp: kStageChunkImages) twice, far below its
    byte limit: three chunks, so the first staging half is packed again while its first chunk's copy and kernel may still run.
    Four distinct scenes with holes, repeated; the images either side of both chunk boundaries and the last equal the restatement."""
    per_chunk = 8192
    n = 2 * per_chunk + 5
    sizes = [(16, 12), (15, 13), (17, 11), (16, 12)]
    scenes = [DS.scene(w, h, seed=70 + k, nans=0.2) for k, (w, h) in enumerate(sizes)]
    want = [DR.refine(im["depth"], g) for im, g in scenes]
    assert all((w != 0).any() and (w == 0).any() for w in want) and not np.array_equal(want[0], want[3])
    h = capi.DepthFilter()
    h.refine([scenes[k % 4][0] for k in range(n)], [scenes[k % 4][1] for k in range(n)])
    assert h.image_count() == n
    for k in (0, per_chunk - 1, per_chunk, 2 * per_chunk - 1, 2 * per_chunk, n - 1):
        same_image(h.read(k), want[k % 4], "image %d" % k)
    h.close()
