"""CPU tests (no GPU needed): uzl_depthfilter_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp:
HandleBase, UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_laserline_handles_cpu.py.  Nothing
here needs a handle on a device, so the tests pass with or without one."""
import ctypes as C
import math

import pytest


def test_null_handle(capi):
    L = capi.lib()
    assert L.uzl_depthfilter_last_error(None) == b"null handle"
    assert L.uzl_depthfilter_destroy(None) is None
    cfg = capi.DepthFilterCfg()
    assert L.uzl_depthfilter_set_config(None, C.byref(cfg)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_refine(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_image_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_read(None, 0, None, C.c_int64(0)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_lift(None, 0, 0, None, None, C.c_double(0.0), None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_to_laserline(None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_create(None, None) == capi.UZL_ERR_BAD_ARG


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_depthfilter" in capi._MORE_HANDLES and "uzl_depthfilter" not in capi._HANDLES


def test_layout_sizes(capi):
    assert C.sizeof(capi.DepthFilterCfg) == 40 and C.sizeof(capi.GuideImage) == 24 and C.sizeof(capi.DepthImage) == 160
    assert capi.DepthFilterCfg.sigma_space.offset == 8 and capi.DepthFilterCfg.use_bilateral_filter.offset == 32
    assert capi.GuideImage.width.offset == 8 and capi.GuideImage.step.offset == 16


def test_defaults_mirror_the_cfg_file_and_the_service_node(capi):
    """FeatureExtraction.cfg:13 (use_bilateral_filter True) and feature_extraction_service_node.cpp:134-140 (r = 3, sigs = 30 and
    sigc = 50 tenths, pr = 2)"""
    c = capi.DepthFilterCfg()
    capi.lib().uzl_depthfilter_cfg_default(C.byref(c))
    assert (c.radius, c.nearest_radius, c.sigma_space, c.sigma_color, c.depth_scale, c.use_bilateral_filter, c.device) == \
        (3, 2, 3.0, 5.0, 1.0, 1, 0)
    assert capi.lib().uzl_abi_version() == 3


BAD = [dict(radius=-1), dict(radius=16), dict(nearest_radius=-1), dict(nearest_radius=8), dict(sigma_space=math.nan),
       dict(sigma_color=math.nan), dict(depth_scale=math.nan), dict(depth_scale=0.0), dict(depth_scale=-1.0)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_argument_errors_come_before_the_device_check(capi, bad):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        capi.DepthFilter(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


GOOD = [dict(radius=0), dict(radius=15), dict(nearest_radius=0), dict(nearest_radius=7), dict(sigma_space=0.0), dict(sigma_color=-2.0),
        dict(use_bilateral_filter=0)]


@pytest.mark.parametrize("good", GOOD, ids=[f"{k}={v}" for b in GOOD for k, v in b.items()])
def test_the_limits_are_allowed(capi, good):
    """the ends of the ranges, and a sigma <= 0 (it becomes 1): on a machine without a GPU these fail at the device check"""
    try:
        capi.DepthFilter(**good).close()
        status = capi.UZL_OK
    except capi.UzlError as e:
        status = e.status
    assert status == (capi.UZL_OK if capi.device_count() > 0 else capi.UZL_ERR_NO_DEVICE)


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        h = capi.DepthFilter()
        h.close()
        with pytest.raises(capi.UzlError) as e:
            capi.DepthFilter(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.DepthFilter()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
