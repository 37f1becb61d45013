"""CPU tests (no GPU needed): uzl_laserline_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp:
HandleBase, UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_handles_cpu.py.  Nothing here
needs a handle on a device, so the tests pass with or without one."""
import ctypes as C
import math

import numpy as np
import pytest


def test_null_handle(capi):
    L = capi.lib()
    assert L.uzl_laserline_last_error(None) == b"null handle"
    assert L.uzl_laserline_destroy(None) is None
    cfg = capi.LaserlineCfg()
    assert L.uzl_laserline_set_config(None, C.byref(cfg)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_extract(None, 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_read(None, 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_to_grid(None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_create(None, None) == capi.UZL_ERR_BAD_ARG


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_laserline" in capi._MORE_HANDLES and "uzl_laserline" not in capi._HANDLES


def test_defaults(capi):
    c = capi.LaserlineCfg()
    capi.lib().uzl_laserline_cfg_default(C.byref(c))
    assert (c.min_height, c.max_height, c.angle_increment, c.range_min, c.range_max, c.depth_scale, c.device) == \
        (0.0, 1.0, math.pi / 360, 0.45, 5.0, 1.0, 0)
    assert C.sizeof(capi.LaserlineCfg) == 56 and C.sizeof(capi.DepthImage) == 160


BAD = [dict(angle_increment=1.0), dict(angle_increment=0.001), dict(angle_increment=0.0), dict(angle_increment=-0.01),
       dict(angle_increment=math.nan), dict(min_height=math.nan), dict(max_height=math.nan), dict(range_min=math.nan),
       dict(range_max=math.nan), dict(depth_scale=math.nan), dict(range_max=0.4), dict(range_min=-0.1), dict(depth_scale=0.0),
       dict(depth_scale=-1.0)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_argument_errors_come_before_the_device_check(capi, bad):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        capi.Laserline(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_the_limits_of_the_angular_grid(capi):
    """n = 8 and n = 4096 are allowed, 7 and 4097 are not; on a machine without a GPU the allowed ones fail at the device check"""
    two_pi = float(np.float32(math.pi) - np.float32(-math.pi))
    for inc, ok in ((two_pi / 7.5, True), (two_pi / 6.5, False), (two_pi / 4095.5, True), (two_pi / 4096.5, False)):
        n = int(np.ceil((np.float32(math.pi) - np.float32(-math.pi)) / np.float32(inc)))
        assert (8 <= n <= 4096) == ok
        try:
            capi.Laserline(angle_increment=inc).close()
            status = capi.UZL_OK
        except capi.UzlError as e:
            status = e.status
        assert (status != capi.UZL_ERR_BAD_ARG) == ok, (inc, n, status)


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        h = capi.Laserline()
        h.close()
        with pytest.raises(capi.UzlError) as e:
            capi.Laserline(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Laserline()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
