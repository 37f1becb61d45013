"""GPU tests of the ORB stage entry (uzl_orb_stage_image, uzl_orb_stage_candidates): what the kernels leave in the handle's work
buffers - every pyramid level of every cell and of the whole image, every mask level, every blurred level over its whole area, the
63 x 63 GIST image and its blur, the FAST candidates of every (cell, level) before the cuts and the cut itself - equals the NumPy
restatement tests/orb_reference.py bit for bit, so a wrong pixel shows whether or not a surviving keypoint happens to sample it, and
a failure names its stage.  Then the statuses of the stage entry, the chunk rule and that reading stages changes no result."""
import ctypes as C

import numpy as np
import pytest

import orb_cases as K
import orb_reference as R
import orb_scenes as S
from test_orb_gpu import PATTERN, SMALL, reference, same, scene

pytestmark = pytest.mark.gpu


def check_stages(capi, h, k, info, cfg, masked=False):
    """every stage of resident image k against the restatement's info for that image"""
    cfg = dict(R.DEFAULTS, **cfg)
    cells, L = cfg["grid_rows"] * cfg["grid_cols"], cfg["n_levels"]
    assert len(info["stages"]) == cells
    for cell, st in enumerate(info["stages"]):
        for l in range(1, L):
            got = h.stage_image(k, capi.ORB_STAGE_LEVEL, cell, l)
            assert np.array_equal(got, st["levels"][l]), ("level image", cell, l, got.shape, st["levels"][l].shape)
            if masked:
                got = h.stage_image(k, capi.ORB_STAGE_MASK, cell, l)
                assert np.array_equal(got, st["masks"][l]), ("mask level", cell, l, got.shape)
        for l in range(L):
            x, y, s, thr = h.stage_candidates(k, cell, l)
            wx, wy, ws = st["candidates"][l]
            assert len(x) == len(wx), ("candidate count", cell, l, len(x), len(wx))
            assert len(set(zip(x.tolist(), y.tolist()))) == len(x), ("a candidate repeats", cell, l)
            assert sorted(zip(x.tolist(), y.tolist(), s.tolist())) == sorted(zip(wx.tolist(), wy.tolist(), ws.tolist())), ("candidates", cell, l)
            assert thr == st["cut"][l], ("cut", cell, l, thr, st["cut"][l])
    counts = [n for _, n, _ in info["level_candidates"]]
    assert counts == [len(st["candidates"][l][0]) for st in info["stages"] for l in range(L)]
    for l in range(L):
        if l:
            got = h.stage_image(k, capi.ORB_STAGE_LEVEL, -1, l)
            assert np.array_equal(got, info["pyramid"][l]), ("whole-image level", l, got.shape, info["pyramid"][l].shape)
        got = h.stage_image(k, capi.ORB_STAGE_BLUR, -1, l)
        want = info["blurred"][l]
        assert got.shape == want.shape, ("blurred level", l, got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, ("blurred level", l, len(bad), bad[:4].tolist())


def test_default_config_and_results_unchanged_by_stage_reads(capi):
    """163 x 157: cells of 81 and 82 by 78 and 79, so every level has cut tiles; reading the stages leaves the results as they were"""
    img = scene(163, 157)
    want, info = reference("rect163x157", img)
    h = capi.Orb(PATTERN)
    h.extract([img], gist_angles=[12.5])
    before, gist = h.read(0), h.gist(0)
    check_stages(capi, h, 0, info, {})
    assert sum(n for _, n, _ in info["level_candidates"]) > 0
    same(h.read(0), before, "after stage reads")
    same(before, want, "163x157")
    assert np.array_equal(h.gist(0), gist) and np.array_equal(gist, R.gist(img, 12.5, PATTERN))
    h.close()


def test_edge_19_four_levels_three_by_two(capi):
    img = scene(201, 187)
    cfg = dict(edge_threshold=19, n_levels=4, grid_rows=3, grid_cols=2, number_of_features=60)
    _, info = reference("rect201x187", img, **cfg)
    assert sum(1 for l, n, _ in info["level_candidates"] if l >= 2 and n > 0) > 0
    h = capi.Orb(PATTERN, **cfg)
    h.extract([img])
    check_stages(capi, h, 0, info, cfg)
    h.close()


def test_tiles_of_one_column_and_one_row(capi):
    """78 x 40 at 1.2: level 1 of the whole image is 65 x 33, one column and one row past the 64 x 32 tile, in the resize and in the
    blur; batched behind a larger image, so that the launch is sized by another image"""
    img = scene(78, 40)
    assert R.level_size(78, 40, 1.2, 1) == (65, 33)
    info = {}
    R.extract(img, PATTERN, info=info)
    big = scene(163, 157)
    h = capi.Orb(PATTERN)
    h.extract([big, img])
    check_stages(capi, h, 1, info, {})
    check_stages(capi, h, 0, reference("rect163x157", big)[1], {})
    h.close()


@pytest.mark.parametrize("name", ["fine_mask", "fine_mask200"])
def test_mask_levels(capi, name):
    case, (want, info) = K.CASES[name], K.reference(name)
    h = capi.Orb(PATTERN, **case["cfg"])
    h.extract([case["img"]], [case["mask"]])
    check_stages(capi, h, 0, info, case["cfg"], masked=True)
    same(h.read(0), want, name)
    with pytest.raises(capi.UzlError) as e:
        h.stage_image(0, capi.ORB_STAGE_MASK, -1, 1)                     # masks are cut per cell
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    h.close()


def test_candidates_and_cuts_at_ties_and_at_the_largest_score(capi):
    img = S.squares(260, 260)
    cfg = dict(number_of_features=20)
    _, info = reference("squares260", img, **cfg)
    assert any(c > 0 for st in info["stages"] for c in st["cut"])          # the cut lies on the tied score
    h = capi.Orb(PATTERN, **cfg)
    h.extract([img])
    check_stages(capi, h, 0, info, cfg)
    for name in ("dots_t254", "inverse_dots_t254", "grid8_share0", "last_level0", "scale2"):
        case, (_, info) = K.CASES[name], K.reference(name)
        h.set_config(**dict(R.DEFAULTS, **case["cfg"]))
        h.extract([case["img"]])
        check_stages(capi, h, 0, info, case["cfg"])
    h.close()
    assert 256 in [c for st in K.reference("grid8_share0")[1]["stages"] for c in st["cut"]]
    assert K.reference("last_level0")[1]["stages"][0]["cut"][2] == 256


@pytest.mark.parametrize("w,h", [(40, 50), (63, 63), (163, 157)])
def test_gist_images(capi, w, h):
    """the source smaller than 63 x 63 (enlarged), equal to it (the identity) and larger"""
    img = scene(w, h)
    o = capi.Orb(PATTERN)
    o.extract([img, np.zeros((0, 0), np.uint8)], gist_angles=[30.0, 0.0])
    small = R.resize(img, 63, 63)
    got = o.stage_image(0, capi.ORB_STAGE_GIST)
    assert got.shape == (63, 63) and np.array_equal(got, small)
    assert np.array_equal(o.stage_image(0, capi.ORB_STAGE_GIST_BLUR), R.blur(small))
    assert o.stage_image(1, capi.ORB_STAGE_GIST).shape == (0, 0) and o.stage_image(1, capi.ORB_STAGE_BLUR, -1, 0).shape == (0, 0)
    assert o.stage_candidates(1, 0, 0)[3] == 0 and len(o.stage_candidates(1, 3, 1)[0]) == 0
    o.close()


def test_statuses(capi):
    L = capi.lib()
    h = capi.Orb(PATTERN)
    i32 = C.c_int32
    w, ht = i32(-7), i32(-7)

    def image(im, what, cell, level, cap=0, out=None):
        return L.uzl_orb_stage_image(h._h, i32(im), i32(what), i32(cell), i32(level), C.c_int64(cap), out, C.byref(w), C.byref(ht))

    def cand(im, cell, level, cap=0, x=None):
        return L.uzl_orb_stage_candidates(h._h, i32(im), i32(cell), i32(level), i32(cap), x, None, None, None)

    assert image(0, capi.ORB_STAGE_LEVEL, 0, 1) == capi.UZL_ERR_STATE and cand(0, 0, 0) == capi.UZL_ERR_STATE   # nothing extracted yet
    assert b"extract" in L.uzl_orb_last_error(h._h)
    img = scene(160, 152)
    h.extract([img])
    before = h.read(0)
    LEVEL, MASK, BLUR, GIST = capi.ORB_STAGE_LEVEL, capi.ORB_STAGE_MASK, capi.ORB_STAGE_BLUR, capi.ORB_STAGE_GIST
    assert image(0, LEVEL, 0, 1) == capi.UZL_OK and (w.value, ht.value) == R.level_size(80, 76, 1.2, 1)
    assert image(0, LEVEL, -1, 1) == capi.UZL_OK and (w.value, ht.value) == R.level_size(160, 152, 1.2, 1)
    for im in (-1, 1):
        assert image(im, LEVEL, 0, 1) == capi.UZL_ERR_BAD_ARG and cand(im, 0, 0) == capi.UZL_ERR_BAD_ARG
    for cell in (-2, 4):
        assert image(0, LEVEL, cell, 1) == capi.UZL_ERR_BAD_ARG and cand(0, cell, 0) == capi.UZL_ERR_BAD_ARG
    assert cand(0, -1, 0) == capi.UZL_ERR_BAD_ARG                          # candidates belong to a cell
    for level in (-1, 2):
        assert image(0, LEVEL, 0, level) == capi.UZL_ERR_BAD_ARG and image(0, BLUR, -1, level) == capi.UZL_ERR_BAD_ARG
        assert cand(0, 0, level) == capi.UZL_ERR_BAD_ARG
    assert image(0, LEVEL, 0, 0) == capi.UZL_ERR_BAD_ARG and image(0, LEVEL, -1, 0) == capi.UZL_ERR_BAD_ARG   # the caller's own input
    assert b"level 0" in L.uzl_orb_last_error(h._h)
    assert image(0, MASK, 0, 0) == capi.UZL_ERR_BAD_ARG
    assert image(0, BLUR, 0, 0) == capi.UZL_ERR_BAD_ARG                    # only the whole image is blurred
    assert image(0, 5, 0, 1) == capi.UZL_ERR_BAD_ARG and image(0, -1, 0, 1) == capi.UZL_ERR_BAD_ARG
    assert image(0, GIST, -1, 0) == capi.UZL_ERR_STATE and image(0, capi.ORB_STAGE_GIST_BLUR, -1, 0) == capi.UZL_ERR_STATE
    assert b"angles" in L.uzl_orb_last_error(h._h)
    assert image(0, MASK, 0, 1) == capi.UZL_ERR_STATE and b"mask" in L.uzl_orb_last_error(h._h)
    buf = np.zeros(160 * 152, np.uint8)
    p = buf.ctypes.data_as(capi.c_u8p)
    assert image(0, BLUR, -1, 0, 160 * 152 - 1, p) == capi.UZL_ERR_TRUNCATED and b"capacity" in L.uzl_orb_last_error(h._h)
    assert image(0, BLUR, -1, 0, -1, p) == capi.UZL_ERR_BAD_ARG
    assert image(0, BLUR, -1, 0, 160 * 152, p) == capi.UZL_OK and (w.value, ht.value) == (160, 152)
    assert np.array_equal(buf.reshape(152, 160), R.blur(img))
    n = cand(0, 3, 0)
    assert n == len(reference("rect160x152", img)[1]["stages"][3]["candidates"][0][0]) and n > 1
    x = np.zeros(n, np.int32)
    assert cand(0, 3, 0, n - 1, x.ctypes.data_as(capi.c_i32p)) == capi.UZL_ERR_TRUNCATED
    assert cand(0, 3, 0, -1, x.ctypes.data_as(capi.c_i32p)) == capi.UZL_ERR_BAD_ARG
    assert cand(0, 3, 0, n, x.ctypes.data_as(capi.c_i32p)) == n and x.min() >= 31
    # a config set after the extract does not change what the buffers hold: the stages keep the extract's grid and level count
    h.set_config(n_levels=4, grid_rows=3, grid_cols=3)
    assert image(0, LEVEL, 0, 2) == capi.UZL_ERR_BAD_ARG and cand(0, 4, 0) == capi.UZL_ERR_BAD_ARG
    assert image(0, LEVEL, 3, 1) == capi.UZL_OK
    same(h.read(0), before, "after refused stage reads")
    h.extract([])
    assert image(0, LEVEL, 0, 1) == capi.UZL_ERR_BAD_ARG                  # an empty set has no image 0
    h.close()


def test_only_the_last_staging_chunk_is_served(capi):
    """1652 images with a 2 x 2 grid go through two chunks (8192 / 5 = 1638 images in the first, test_orb_gpu.py): the work buffers
    hold the second; an image of the first is refused and says why"""
    tiny = np.full((8, 8), 200, np.uint8)
    tiny[2:5, 3:6] = 30
    real = scene(163, 157)
    h = capi.Orb(PATTERN, **SMALL)
    h.extract([tiny] * 1650 + [scene(160, 152), real])
    want, info = reference("rect163x157", real, **SMALL)
    for k in (0, 1637):
        with pytest.raises(capi.UzlError) as e:
            h.stage_image(k, capi.ORB_STAGE_BLUR, -1, 0)
        assert e.value.status == capi.UZL_ERR_STATE and "chunk" in str(e.value)
        with pytest.raises(capi.UzlError) as e:
            h.stage_candidates(k, 0, 0)
        assert e.value.status == capi.UZL_ERR_STATE and "chunk" in str(e.value)
    assert np.array_equal(h.stage_image(1638, capi.ORB_STAGE_BLUR, -1, 0), R.blur(tiny))
    assert np.array_equal(h.stage_image(1649, capi.ORB_STAGE_LEVEL, -1, 1), R.pyramid(tiny, 2, 1.2)[1])
    check_stages(capi, h, 1651, info, SMALL)
    same(h.read(1651), want, "image 1651")
    assert h.count(0) == 0                                               # the results of the first chunk are still there
    h.close()
