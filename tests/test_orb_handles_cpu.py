"""CPU tests (no GPU needed): uzl_orb_* through the lifecycle and error path every uzl_* handle shares, in the manner of
tests/test_depthfilter_handles_cpu.py.  Nothing here needs a handle on a device, so the tests pass with or without one."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import orb_scenes as S


def test_null_handle(capi):
    L = capi.lib()
    assert L.uzl_orb_last_error(None) == b"null handle"
    assert L.uzl_orb_destroy(None) is None
    cfg = capi.OrbCfg()
    assert L.uzl_orb_set_config(None, C.byref(cfg)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_extract(None, 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_image_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_count(None, 0) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_read(None, 0, 0, None, None, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_gist(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_lift(None, 0, None, 0, C.c_double(0.0), None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_orb_create(None, None, None) == capi.UZL_ERR_BAD_ARG


def test_null_handle_at_the_stage_entry(capi):
    L = capi.lib()
    w, h = C.c_int32(-7), C.c_int32(-7)
    for what in (capi.ORB_STAGE_LEVEL, capi.ORB_STAGE_MASK, capi.ORB_STAGE_BLUR, capi.ORB_STAGE_GIST, capi.ORB_STAGE_GIST_BLUR):
        assert L.uzl_orb_stage_image(None, 0, what, 0, 1, C.c_int64(0), None, C.byref(w), C.byref(h)) == capi.UZL_ERR_BAD_ARG
    assert (w.value, h.value) == (-7, -7)                                  # a refused call writes nothing
    assert L.uzl_orb_stage_candidates(None, 0, 0, 0, 0, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert (capi.ORB_STAGE_LEVEL, capi.ORB_STAGE_MASK, capi.ORB_STAGE_BLUR, capi.ORB_STAGE_GIST, capi.ORB_STAGE_GIST_BLUR) == (0, 1, 2, 3, 4)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uzl_mi355x.h")).read()
    for k, name in enumerate(("LEVEL", "MASK", "BLUR", "GIST", "GIST_BLUR")):
        assert re.search(r"#define UZL_ORB_STAGE_%s\s+%d\b" % (name, k), src), name


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_orb" in capi._MORE_HANDLES and "uzl_orb" not in capi._HANDLES


def test_layout(capi):
    assert C.sizeof(capi.OrbCfg) == 40
    assert capi.OrbCfg.scale_factor.offset == 16 and capi.OrbCfg.gist_size.offset == 32 and capi.OrbCfg.device.offset == 36


def test_defaults_equal_the_cited_values(capi):
    """feature_extraction_service.launch:7 (300 features), feature_extraction_core.cpp:65 (1.2f, 2 levels, edge 31, patch 31, FAST 5),
    :84 (2 x 2 grid), :141 (63)"""
    c = capi.OrbCfg()
    capi.lib().uzl_orb_cfg_default(C.byref(c))
    assert (c.number_of_features, c.grid_rows, c.grid_cols, c.n_levels, c.edge_threshold, c.patch_size, c.fast_threshold, c.gist_size,
            c.device) == (300, 2, 2, 2, 31, 31, 5, 63, 0)
    assert np.float32(c.scale_factor) == np.float32(1.2)
    assert capi.lib().uzl_abi_version() == 3


BAD = [dict(patch_size=30), dict(patch_size=32), dict(edge_threshold=18), dict(n_levels=0), dict(n_levels=9), dict(scale_factor=1.0),
       dict(scale_factor=2.5), dict(scale_factor=math.nan), dict(fast_threshold=0), dict(fast_threshold=255),
       dict(number_of_features=0), dict(grid_rows=0), dict(grid_rows=9), dict(grid_cols=0), dict(grid_cols=9), dict(gist_size=64)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_argument_errors_come_before_the_device_check(capi, bad):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        capi.Orb(S.pattern(), **bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


@pytest.mark.parametrize("what", ["null", "x=16", "y=-16"])
def test_pattern_errors_come_before_the_device_check(capi, what):
    pat = S.pattern()
    if what == "x=16":
        pat[511, 0] = 16
    if what == "y=-16":
        pat[0, 1] = -16
    with pytest.raises(capi.UzlError) as e:
        capi.Orb(None if what == "null" else pat)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


GOOD = [dict(), dict(edge_threshold=19), dict(n_levels=1), dict(n_levels=8), dict(scale_factor=2.0), dict(fast_threshold=1),
        dict(fast_threshold=254), dict(number_of_features=1), dict(grid_rows=8, grid_cols=8)]


@pytest.mark.parametrize("good", GOOD, ids=[",".join(f"{k}={v}" for k, v in g.items()) or "defaults" for g in GOOD])
def test_a_good_config_gets_past_the_checks(capi, good):
    """Without a device the create then reports UZL_ERR_NO_DEVICE (there is no CPU fallback); with one it succeeds."""
    pat = S.pattern()
    pat[0] = (15, -15)                               # the ends of the admitted range
    if capi.device_count() > 0:
        capi.Orb(pat, **good).close()
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Orb(pat, **good)
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
