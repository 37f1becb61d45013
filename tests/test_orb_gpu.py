"""GPU tests of uzl_orb_* (ORB keypoints, descriptors and binary GIST): every field - count, u, v, response, angle, octave, desc,
gist - equals the NumPy restatement tests/orb_reference.py bit for bit, at the smallest sizes at which each branch lives (both levels
inside the border, unequal cells and cut tiles, a level the border empties, no keypoints, 0 x 0) and once at 640 x 480; both cuts are
shown to be exercised, ties are all kept, a saturated image and a mask are followed, batching and repetition change nothing; the GIST
goes into uzl_gist_* unchanged; uzl_orb_lift equals uzl_depthfilter_lift and its arrays go into the estimator; the error paths."""
import ctypes as C

import numpy as np
import pytest

import orb_reference as R
import orb_scenes as S

pytestmark = pytest.mark.gpu

F32 = np.float32
PATTERN = S.pattern()
SMALL = dict(number_of_features=4)          # 8 per cell and level pair: small images exceed both cuts
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def reference(name, img, mask=None, **cfg):
    """the restatement's result for a scene, computed once"""
    key = (name, tuple(sorted(cfg.items())), mask is not None)
    if key not in _cache:
        info = {}
        _cache[key] = (R.extract(img, PATTERN, mask=mask, info=info, **cfg), info)
    return _cache[key]


def same(got, want, what=""):
    assert len(got["u"]) == len(want["u"]), (what, len(got["u"]), len(want["u"]))
    for f in ("u", "v", "response", "angle"):
        d = np.nonzero(bits(got[f]) != bits(want[f]))[0]
        assert len(d) == 0, "%s: %s differs at %s: %s vs %s" % (what, f, d[:5].tolist(), got[f][d[:5]].tolist(), want[f][d[:5]].tolist())
    assert np.array_equal(got["octave"], want["octave"]), what
    d = np.nonzero((got["desc"] != want["desc"]).any(axis=1))[0]
    assert len(d) == 0, "%s: %d descriptors differ, first %s" % (what, len(d), d[:5].tolist())


def scene(w, h):
    return S.rectangles(w, h, seed=1000 + w)


def run(capi, images, masks=None, angles=None, **cfg):
    h = capi.Orb(PATTERN, **cfg)
    h.extract(images, masks, angles)
    assert h.image_count() == len(images)
    out = [h.read(k) for k in range(len(images))]
    gists = [h.gist(k) for k in range(len(images))] if angles is not None else None
    h.close()
    return out, gists


@pytest.mark.parametrize("w,h", [(160, 152), (163, 157), (144, 144), (64, 64)])
def test_small_sizes(capi, w, h):
    img = scene(w, h)
    for cfg in (SMALL, {}):
        want, info = reference("rect%dx%d" % (w, h), img, **cfg)
        got, _ = run(capi, [img], **cfg)
        same(got[0], want, "%dx%d %s" % (w, h, cfg))
    _, info = reference("rect%dx%d" % (w, h), img, **SMALL)
    if (w, h) == (160, 152):
        # both levels of every cell survive the border, and both cuts are exercised
        assert all(R.level_size(w // 2, h // 2, 1.2, 1)[k] > 62 for k in (0, 1))
        assert any(n > n_l for _, n, n_l in info["level_candidates"]) and any(n > share for n, share in info["cell_candidates"])
    if (w, h) == (144, 144):
        assert R.level_size(72, 72, 1.2, 1) == (60, 60) and all(n == 0 for l, n, _ in info["level_candidates"] if l == 1)
    if (w, h) == (64, 64):
        assert len(got[0]["u"]) == 0


def test_edge_19_and_more_levels(capi):
    """the smallest admitted border, four levels, a 3 x 2 grid: descriptors of the upper levels read past their level image"""
    img = scene(201, 187)
    cfg = dict(edge_threshold=19, n_levels=4, grid_rows=3, grid_cols=2, number_of_features=60)
    want, _ = reference("rect201x187", img, **cfg)
    assert set(want["octave"].tolist()) >= {0, 1, 2}
    got, _ = run(capi, [img], **cfg)
    same(got[0], want)


def test_constant_and_empty_images(capi):
    got, gists = run(capi, [np.full((152, 160), 90, np.uint8), np.zeros((0, 0), np.uint8)], angles=[0.0, 10.0])
    assert len(got[0]["u"]) == 0 and len(got[1]["u"]) == 0 and got[1]["desc"].shape == (0, 32)
    assert np.array_equal(gists[0], R.gist(np.full((152, 160), 90, np.uint8), 0.0, PATTERN))
    assert not gists[1].any()
    h = capi.Orb(PATTERN)
    h.extract([])
    assert h.image_count() == 0
    h.close()


def test_vga(capi):
    img = scene(640, 480)
    want, info = reference("rect640x480", img)
    # the restatement finds more than n_l candidates on a level and more than its share in a cell: both cuts are exercised
    assert any(n >= n_l + 1 for _, n, n_l in info["level_candidates"]) and any(n > share for n, share in info["cell_candidates"])
    assert len(want["u"]) >= 300 and set(want["octave"].tolist()) == {0, 1}
    got, _ = run(capi, [img])
    same(got[0], want, "640x480")


def test_ties_are_all_kept(capi):
    img = S.squares(260, 260)
    cfg = dict(number_of_features=20)
    want, info = reference("squares260", img, **cfg)
    r, counts = np.unique(want["response"][want["octave"] == 0], return_counts=True)
    n_l = R.n_per_level(40, 1.2, 2)
    assert counts.max() > 4 * n_l[0], (r, counts)                     # more equal-score corners on level 0 than four cells may keep
    got, _ = run(capi, [img], **cfg)
    same(got[0], want, "squares")
    keys = list(zip(got[0]["octave"].tolist(), (-got[0]["response"]).tolist(), got[0]["v"].tolist(), got[0]["u"].tolist()))
    assert keys == sorted(keys)


def test_saturated_image(capi):
    img = S.saturated(200, 180, seed=9)
    assert set(np.unique(img).tolist()) == {0, 255}
    want, _ = reference("saturated", img, **SMALL)
    want_all, _ = reference("saturated", img)
    assert len(want_all["u"]) > 0 and want_all["response"].max() == 254
    got, _ = run(capi, [img, img], **SMALL)
    same(got[0], want)
    got, _ = run(capi, [img])
    same(got[0], want_all)


def test_mask(capi):
    w, h = 240, 200
    img, mask = scene(w, h), S.half_mask(w, h)
    assert mask[h // 2 - 1, :].min() == 0 and mask[h // 2 - 1, :].max() == 255 and mask[h - 1, :].max() == 255   # the edge crosses the cell border
    want, _ = reference("mask", img, mask=mask)
    free, _ = reference("mask", img)
    assert 0 < len(want["u"]) < len(free["u"])
    got, _ = run(capi, [img], masks=[mask])
    same(got[0], want, "masked")
    lv = got[0]["octave"] == 0
    assert (mask[got[0]["v"][lv].astype(int), got[0]["u"][lv].astype(int)] != 0).all()
    got, _ = run(capi, [img], masks=[np.full_like(mask, 255)])
    same(got[0], free, "mask of 255")


def test_batching_and_replacement(capi):
    sizes = [(160, 152), (163, 157), (0, 0), (144, 144), (201, 187)]
    images = [scene(w, h) if w else np.zeros((0, 0), np.uint8) for w, h in sizes]
    h = capi.Orb(PATTERN, **SMALL)
    h.extract(images, gist_angles=[0.0, 90.0, 5.0, -17.5, 720.25])
    together = [h.read(k) for k in range(5)]
    gists = [h.gist(k) for k in range(5)]
    for k, (w, hh) in enumerate(sizes):
        h.extract([images[k]], gist_angles=[[0.0, 90.0, 5.0, -17.5, 720.25][k]])        # a second extract replaces the first
        assert h.image_count() == 1
        same(h.read(0), together[k], "image %d alone" % k)
        assert np.array_equal(h.gist(0), gists[k])
        if w:
            same(together[k], reference("rect%dx%d" % (w, hh), images[k], **SMALL)[0], "image %d" % k)
    # rows with padding give what compact rows give
    wide = np.zeros((152, 200), np.uint8)
    wide[:, :160] = images[0]
    h.extract([wide[:, :160]])
    same(h.read(0), together[0], "strided rows")
    with pytest.raises(capi.UzlError) as e:
        h.gist(0)                                                      # the last extract had no angles
    assert e.value.status == capi.UZL_ERR_STATE
    h.close()


def test_more_images_than_one_staging_chunk(capi):
    """a chunk holds at most 8192 / (cells + 1) = 1638 images (uzl_orb.hip): the images behind that mark go through a second chunk
    with buffers and offsets of its own and give what they give alone"""
    tiny = np.full((8, 8), 200, np.uint8)
    tiny[2:5, 3:6] = 30
    real = [scene(160, 152), scene(163, 157)]
    images = [tiny] * 1650 + real
    angles = [float(k % 360) for k in range(len(images))]
    h = capi.Orb(PATTERN, **SMALL)
    h.extract(images, gist_angles=angles)
    assert h.image_count() == 1652
    for k in (0, 1637, 1638, 1649):
        assert h.count(k) == 0 and np.array_equal(h.gist(k), R.gist(tiny, angles[k], PATTERN)), k
    for k, (w, hh) in zip((1650, 1651), ((160, 152), (163, 157))):
        same(h.read(k), reference("rect%dx%d" % (w, hh), real[k - 1650], **SMALL)[0], "image %d" % k)
        assert np.array_equal(h.gist(k), R.gist(real[k - 1650], angles[k], PATTERN))
    h.close()


ANGLES = [0.0, 90.0, 359.9, -17.5, 720.25]


@pytest.mark.parametrize("w,h", [(63, 63), (640, 480)])
def test_gist(capi, w, h):
    img = scene(w, h)
    if (w, h) == (63, 63):
        assert np.array_equal(R.resize(img, 63, 63), img)             # the resize is the identity
    _, gists = run(capi, [img] * len(ANGLES), angles=ANGLES)
    for a, g in zip(ANGLES, gists):
        assert np.array_equal(g, R.gist(img, a, PATTERN)), a
    assert len(set(g.tobytes() for g in gists)) >= 3                  # the angle matters (0, 359.9 and 720.25 may sample the same pixels)


def test_gist_goes_into_the_place_recogniser(capi):
    imgs = [scene(160, 152), scene(163, 157), scene(201, 187)]
    _, gists = run(capi, imgs, angles=[0.0, 3.0, -2.0])
    g = capi.Gist()
    for k, d in enumerate(gists):
        g.add(d, k * 10 ** 9)
    d_u8 = np.frombuffer(gists[1].tobytes(), np.uint8)
    L = capi.lib()
    out = np.zeros(8, np.int32); n = C.c_int32(); idx = C.c_int32()
    rc = L.uzl_gist_search_and_add(g._h, d_u8.ctypes.data_as(capi.c_u8p), C.c_int32(32), C.c_int64(10 ** 12), C.c_int32(8),
                                   out.ctypes.data_as(capi.c_i32p), C.byref(n), C.byref(idx))
    assert rc == capi.UZL_OK and idx.value == 3
    found = out[:n.value].tolist()
    assert 1 in found                                                 # the stored place with these very bytes: distance 0
    dist = [int(np.unpackbits(gists[k] ^ gists[1]).sum()) for k in range(3)]
    assert dist[1] == 0 and min(dist[0], dist[2]) > 0
    g.close()


def round_half_away(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5)).astype(np.int32)


def test_lift_and_the_estimator(capi):
    """grey + depth image -> uzl_frame without the keypoints leaving the device"""
    import depthfilter_scenes as DS
    w, h = 320, 240
    grey = [scene(w, h), np.roll(scene(w, h), 3, axis=1)]
    depth = [DS.scene(w, h, seed=70)[0], DS.scene(w, h, seed=70)[0]]
    df = capi.DepthFilter()
    df.refine(depth, grey)
    orb = capi.Orb(PATTERN)
    orb.extract(grey)
    on_device, on_host = capi.Match(), capi.Match()
    ids = []
    for k in range(2):
        kp = orb.read(k)
        n = len(kp["u"])
        assert n > 100
        pos, valid = orb.lift(k, df, k, 10.0)
        u, v = round_half_away(kp["u"]), round_half_away(kp["v"])
        assert (np.abs(u - kp["u"]) <= 0.5).all() and (u != np.floor(kp["u"])).any()
        pos_h, valid_h = df.lift(k, u, v, 10.0)
        assert pos.shape == (3, n) and 0 < valid.sum() <= n
        assert np.array_equal(pos.view(np.uint64), np.ascontiguousarray(pos_h).view(np.uint64)) and np.array_equal(valid, valid_h)
        ids.append((on_device.add_frame(kp["desc"], pos, valid), on_host.add_frame(kp["desc"].copy(), pos_h.copy(), valid_h.copy())))
    a, _ = on_device.estimate([(ids[0][0], ids[1][0])])
    b, _ = on_host.estimate([(ids[0][1], ids[1][1])])
    assert a[0]["n_matches"] > 0 and a.tobytes() == b.tobytes()
    # a filter image of another size, an image outside the set, a null filter
    L = capi.lib()
    assert L.uzl_orb_lift(orb._h, 0, None, 0, C.c_double(0.0), None, None) == capi.UZL_ERR_BAD_ARG
    with pytest.raises(capi.UzlError) as e:
        orb.lift(0, df, 2)
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    for x in (on_device, on_host, orb, df):
        x.close()


def test_error_paths(capi):
    L = capi.lib()
    h = capi.Orb(PATTERN)
    f32p = C.POINTER(C.c_float)
    assert L.uzl_orb_image_count(h._h) == capi.UZL_ERR_STATE            # nothing extracted yet
    assert L.uzl_orb_count(h._h, 0) == capi.UZL_ERR_STATE
    assert L.uzl_orb_read(h._h, 0, 0, None, None, None, None, None, None) == capi.UZL_ERR_STATE
    assert L.uzl_orb_gist(h._h, 0, None) == capi.UZL_ERR_STATE
    img = scene(160, 152)
    h.extract([img])
    n = h.count(0)
    assert n > 1
    assert L.uzl_orb_count(h._h, 1) == capi.UZL_ERR_BAD_ARG and L.uzl_orb_count(h._h, -1) == capi.UZL_ERR_BAD_ARG
    u = np.zeros(n, F32)
    assert L.uzl_orb_read(h._h, 1, n, u.ctypes.data_as(f32p), None, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_read(h._h, 0, -1, u.ctypes.data_as(f32p), None, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_read(h._h, 0, n - 1, u.ctypes.data_as(f32p), None, None, None, None, None) == capi.UZL_ERR_TRUNCATED
    assert b"capacity" in L.uzl_orb_last_error(h._h)
    assert L.uzl_orb_read(h._h, 0, 0, None, None, None, None, None, None) == n       # all NULL only asks for the count
    assert L.uzl_orb_read(h._h, 0, n, u.ctypes.data_as(f32p), None, None, None, None, None) == n
    before = h.read(0)
    # what extract refuses leaves the resident results as they were
    arr, keep = capi.DepthFilter.pack_guides([img])
    marr, mkeep = capi.DepthFilter.pack_guides([np.full((10, 10), 255, np.uint8)])
    assert L.uzl_orb_extract(h._h, 1, arr, marr, None) == capi.UZL_ERR_BAD_ARG        # a mask of another size
    assert L.uzl_orb_extract(h._h, -1, arr, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_extract(h._h, 1, None, None, None) == capi.UZL_ERR_BAD_ARG
    nan = np.array([np.nan], F32)
    assert L.uzl_orb_extract(h._h, 1, arr, None, nan.ctypes.data_as(f32p)) == capi.UZL_ERR_BAD_ARG
    arr[0].step = 100
    assert L.uzl_orb_extract(h._h, 1, arr, None, None) == capi.UZL_ERR_BAD_ARG        # a step smaller than a row
    arr[0].step = 160; arr[0].data = None
    assert L.uzl_orb_extract(h._h, 1, arr, None, None) == capi.UZL_ERR_BAD_ARG
    same(h.read(0), before, "after refused extracts")
    h.close()
