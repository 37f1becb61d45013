"""GPU tests of uzl_orb_* across the configs check_cfg admits, away from the defaults: for every case of tests/orb_cases.py - the
FAST threshold at 1, 40, 253 and 254, scale factors 1.05, 1.5 and 2.0 on up to eight levels, grids of 1 x 1, 1 x 2 and 8 x 8, a
per-cell and a per-level share of zero, a pattern that reaches +-15 and reads outside a level-0 image, orientation patches whose
angle is exactly 0, 90, 180, 270 or on a diagonal, masks of 0 / 1 and 0 / 200 in fields finer than a pyramid step - count, u, v,
response, angle, octave, desc and gist equal the NumPy restatement bit for bit.  What each case exercises is asserted on the
restatement in tests/test_orb_reference.py; here the device is held to it, alone, in batches and across uzl_orb_set_config."""
import numpy as np
import pytest

import orb_cases as K
import orb_reference as R
import orb_scenes as S
from test_orb_gpu import PATTERN, bits, run, same, scene

pytestmark = pytest.mark.gpu

F32 = np.float32
ANGLE = 33.25
EMPTY = np.zeros((0, 0), np.uint8)


@pytest.mark.parametrize("name", [n for n in K.CASES if K.CASES[n]["pattern"] is None])
def test_case_alone(capi, name):
    case, (want, _) = K.CASES[name], K.reference(name)
    got, gists = run(capi, [case["img"]], None if case["mask"] is None else [case["mask"]], [ANGLE], **case["cfg"])
    same(got[0], want, name)
    assert np.array_equal(gists[0], R.gist(case["img"], ANGLE, PATTERN))


def test_pattern_15(capi):
    """some level-0 descriptors read outside the image: the unblurred image at the reflect-101 index"""
    case, (want, info) = K.CASES["pattern15"], K.reference("pattern15")
    h = capi.Orb(case["pattern"], **case["cfg"])
    h.extract([case["img"], EMPTY], gist_angles=[ANGLE, 0.0])
    got = h.read(0)
    same(got, want, "pattern15")
    out = np.nonzero(np.array(info["outside"]) > 0)[0]
    assert len(out) >= 1 and np.array_equal(got["desc"][out], want["desc"][out])
    assert np.array_equal(h.gist(0), R.gist(case["img"], ANGLE, case["pattern"]))
    h.close()


def test_satellite_angles(capi):
    case, (want, _) = K.CASES["satellites"], K.reference("satellites")
    _, where = S.satellites()
    got, _ = run(capi, [case["img"]], **case["cfg"])
    got = got[0]
    same(got, want, "satellites")
    at = {(int(u), int(v)): k for k, (u, v) in enumerate(zip(got["u"], got["v"]))}
    d = R.fast_atan2(F32(1), F32(1))
    exact = {None: F32(0), (10, 0): F32(0), (0, 10): F32(90), (-10, 0): F32(180), (0, -10): F32(270), (7, 7): d, (-7, 7): F32(180) - d,
             (-7, -7): F32(360) - (F32(180) - d), (7, -7): F32(360) - d}
    for x, y, off in where:
        k = at[(x, y)]
        if off in exact:
            assert bits(got["angle"][k:k + 1])[0] == bits(np.array([exact[off]], F32))[0], (off, got["angle"][k], exact[off])
            assert np.array_equal(got["desc"][k], want["desc"][k]), off
    assert len(where) == len(got["u"]) == 10


def first_with(cfg):
    return [n for n in K.CASES if K.CASES[n]["cfg"] == cfg and K.CASES[n]["mask"] is None and K.CASES[n]["pattern"] is None]


def test_batches_and_set_config(capi):
    """one handle, a config after the other through uzl_orb_set_config; every case of a config in one extract, between images of
    other sizes and a 0 x 0 image: batching changes nothing, and each extract follows the config set last"""
    others = [scene(64, 64), EMPTY, scene(144, 144)]
    order = ["dots_t253", "scale2", "grid8_share0", "grid8", "scale105", "last_level0", "rect160_t1", "scale15", "satellites", "rect160_t40"]
    h = capi.Orb(PATTERN)
    for lead in order:
        cfg = K.CASES[lead]["cfg"]
        names = first_with(cfg)
        assert lead in names
        images = [others[0]] + [K.CASES[n]["img"] for n in names] + others[1:]
        h.set_config(**dict(R.DEFAULTS, **cfg))
        h.extract(images, gist_angles=[ANGLE] * len(images))
        assert h.image_count() == len(images) and h.count(len(names) + 1) == 0
        for k, n in enumerate(names):
            same(h.read(k + 1), K.reference(n)[0], "%s in the batch of %s" % (n, lead))
            assert np.array_equal(h.gist(k + 1), R.gist(K.CASES[n]["img"], ANGLE, PATTERN))
    h.close()
    assert len(first_with(K.CASES["dots_t253"]["cfg"])) == 2


def test_masked_batch_with_an_empty_image(capi):
    a, b = K.CASES["fine_mask"], K.CASES["fine_mask200"]
    assert a["cfg"] == b["cfg"] and np.array_equal(a["img"], b["img"])
    got, gists = run(capi, [a["img"], EMPTY, b["img"]], [a["mask"], EMPTY, b["mask"]], [ANGLE, 1.0, ANGLE], **a["cfg"])
    same(got[0], K.reference("fine_mask")[0], "fine_mask in a batch")
    same(got[2], K.reference("fine_mask200")[0], "fine_mask200 in a batch")
    assert len(got[1]["u"]) == 0 and not gists[1].any()
    assert np.array_equal(gists[0], gists[2]) and gists[0].any()
