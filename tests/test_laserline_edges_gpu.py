"""GPU tests of the laser-line kernels at planted edges (scenes: tests/laserline_edge_scenes.py; that each edge really occurs in
them is asserted on the CPU by test_laserline_edges_reference.py): points of exact f32 coordinates one and two ulps either side of
bin boundaries, at the +-pi seam, on the axes, at the origin and where the atan2f guess misses, on four angular grids; non-finite
coordinates; height and depth limits; columns that walk through the bins row by row within one lane (sticky bin, flushes, the seam
across the rows, returns, dropped pixels, partial bands, band_rows = 9); every branch of the merge and the bounds of the centre;
and the same walks through the depth filter's device path.  Every comparison is bit for bit against laserline_reference.extract."""
import numpy as np
import pytest

import depthfilter_reference as DR
import laserline_edge_scenes as ES
from test_laserline_gpu import bits, check, same

pytestmark = pytest.mark.gpu

F32 = np.float32
GRID_IDS = [str(n) for n in ES.GRIDS]
WALKS = [(u16, name) for u16 in (False, True) for name in ES.walk_scenes(u16)]


@pytest.mark.parametrize("n", ES.GRIDS, ids=GRID_IDS)
def test_planted_points(capi, n):
    """boundary neighbours, seam, axes, origin and guess misses: one image and one scan per point"""
    images = ES.planted_images(n)
    assert 300 < len(images) < 700
    r, i, c = check(capi, images, angle_increment=ES.GRIDS[n])
    points = ((r < F32(6)) | (i > 0)).sum(1)                                # a point beyond hi leaves only its intensity
    assert points.max() == 1 and (points == 0).sum() == 4                   # only the four origins are dropped
    # all of them in one group as well: the merge over hundreds of cameras, near and far points sharing bins
    check(capi, [dict(im, group=0) for im in images], angle_increment=ES.GRIDS[n], range_min=0.0)


@pytest.mark.parametrize("n", ES.GRIDS, ids=GRID_IDS)
def test_non_finite_coordinates(capi, n):
    r, i, c = check(capi, list(ES.NONFINITE.values()), angle_increment=ES.GRIDS[n])
    assert (r == F32(6)).all() and np.isinf(i).sum() == 9 and (c == 0).all()


def test_height_limits(capi):
    for (lo, hi), cases in ES.HEIGHTS.items():
        r, _, _ = check(capi, ES.height_images((lo, hi)), min_height=lo, max_height=hi)
        assert ((r < F32(6)).sum(1) == np.array([k for _, k in cases])).all()


@pytest.mark.parametrize("enc", ["f32", "u16"])
def test_depth_validity(capi, enc):
    images = ES.depth_validity_images()[enc]
    for scale in ES.DEPTH_SCALES[enc]:
        with np.errstate(over="ignore"):
            check(capi, images, depth_scale=scale)
            check(capi, [dict(im, group=0) for im in images], depth_scale=scale)


@pytest.mark.parametrize("u16,name", WALKS, ids=["%s %s" % ("u16" if u else "f32", nm) for u, nm in WALKS])
def test_column_walks(capi, u16, name):
    h = capi.Laserline(**ES.WINDOW)
    same(h.extract([ES.walk_scenes(u16)[name]]), ES.expected("walk", name, u16))
    h.close()


def test_column_walks_in_one_call_and_planes(capi):
    """every walk of both encodings as the images of one call (another chunk layout, the same bands), then the one-bin planes"""
    images, want = [], []
    for u16, name in WALKS:
        images.append(ES.walk_scenes(u16)[name])
        want.append(ES.expected("walk", name, u16))
    for name, im in ES.plane_scenes().items():
        images.append(im)
        want.append(ES.expected("plane", name))
        assert (want[-1][0] < F32(6)).sum() == 1
    h = capi.Laserline(**ES.WINDOW)
    same(h.extract(images), tuple(np.concatenate([w[k] for w in want]) for k in range(3)))
    h.close()


def test_bands_of_nine_rows(capi):
    w, rows, copies = ES.BAND9
    im = ES.band9_image()
    assert im["depth"].shape == (rows, w) and ES.band_rows(rows * copies) == 9
    want = ES.expected("band9")
    h = capi.Laserline(**ES.WINDOW)
    got = h.extract([dict(im, group=k) for k in range(copies)])
    same(got, tuple(np.concatenate([x] * copies) for x in want))
    h.close()
    assert (want[0] < F32(6)).sum() > 100


@pytest.mark.parametrize("n", [720, 4096], ids=["720", "4096"])
def test_merge_truth_table(capi, n):
    for cfg in ES.merge_cfgs():
        images, groups = ES.merge_images(cfg)
        r, i, c = check(capi, images, angle_increment=ES.GRIDS[n], **cfg)
        assert len(r) == len(groups)
        if cfg == ES.MERGE_CFG:
            assert (r == 0).any() and np.isinf(i).any()


def test_centre_bounds(capi):
    images = ES.grouped(ES.centre_groups().values())
    r, i, c = check(capi, images, **ES.CENTRE_CFG)
    assert (c[2:] == 0).all() and (c[:2, :2] != 0).all()
    check(capi, images, range_min=0.0, range_max=5.0)
    check(capi, images, range_min=2.0, range_max=2.0)
    check(capi, images, range_min=float(ES.up(0.45)), range_max=float(ES.down(5.0)))


def test_every_beam_counted_at_4096(capi):
    images, want = ES.every_beam()
    h = capi.Laserline(angle_increment=ES.GRIDS[4096])
    same(h.extract(images), want)
    h.close()


def test_walks_through_the_depth_filter(capi):
    """filter off, f32, depth_scale 1: the resident images are the depths bit for bit, and uzl_depthfilter_to_laserline bins them
    through the same kernel with step = 4 width"""
    names = list(ES.walk_scenes(False))
    images = [ES.walk_scenes(False)[nm] for nm in names] + list(ES.plane_scenes().values())
    for im in images[:3]:
        assert np.array_equal(bits(DR.refine(im["depth"], None, use_bilateral_filter=0)), bits(im["depth"]))
    want = [ES.expected("walk", nm, False) for nm in names] + [ES.expected("plane", nm) for nm in ES.plane_scenes()]
    f, line = capi.DepthFilter(use_bilateral_filter=0), capi.Laserline(**ES.WINDOW)
    f.refine(images)
    assert np.array_equal(bits(f.read(0)), bits(images[0]["depth"]))
    got = f.to_laserline(line)
    same(got, tuple(np.concatenate([w[k] for w in want]) for k in range(3)))
    for x in (f, line):
        x.close()
