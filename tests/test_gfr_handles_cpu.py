"""CPU tests (no GPU needed): uzl_gfr_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp: HandleBase,
UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_laserline_handles_cpu.py.  Nothing here needs
a handle on a device, so the tests pass with or without one."""
import ctypes as C
import math

import pytest


def test_null_handle(capi):
    L = capi.lib()
    assert L.uzl_gfr_last_error(None) == b"null handle"
    assert L.uzl_gfr_destroy(None) is None
    n = C.c_int32()
    assert L.uzl_gfr_search_and_add(None, None, 0, 0, 2, C.c_int64(0), 0, None, C.byref(n), None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_add(None, None, 0, 0, 2, C.c_int64(0), None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_search(None, None, 0, 0, 2, C.c_int64(0), -1, 0, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_remove(None, 0) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_feature_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_link_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_last_matches(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_last_votes(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_get_feature(None, 0, None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_create(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gfr_cfg_default(None) is None


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_gfr" in capi._MORE_HANDLES and "uzl_gfr" not in capi._HANDLES


def test_defaults(capi):
    c = capi.GfrCfg()
    capi.lib().uzl_gfr_cfg_default(C.byref(c))
    assert (c.T, c.k_nearest_neighbors, c.max_distance, c.device, c.min_time_gap, c.initial_features) == (10.0, 10, 40, 0, 5.0, 65536)
    assert C.sizeof(capi.GfrCfg) == 40
    assert (capi.GfrCfg.T.offset, capi.GfrCfg.k_nearest_neighbors.offset, capi.GfrCfg.max_distance.offset, capi.GfrCfg.device.offset,
            capi.GfrCfg.min_time_gap.offset, capi.GfrCfg.initial_features.offset) == (0, 8, 12, 16, 24, 32)


BAD = [dict(T=math.nan), dict(min_time_gap=math.nan), dict(k_nearest_neighbors=-1), dict(k_nearest_neighbors=257), dict(max_distance=0),
       dict(max_distance=-40), dict(max_distance=513), dict(initial_features=0), dict(initial_features=-1),
       dict(initial_features=2**30 + 1)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_argument_errors_come_before_the_device_check(capi, bad):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        capi.Gfr(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


@pytest.mark.parametrize("ok", [dict(k_nearest_neighbors=0), dict(k_nearest_neighbors=256), dict(max_distance=1), dict(max_distance=512),
                                dict(T=-1.0), dict(T=math.inf), dict(initial_features=1)], ids=str)
def test_the_limits_themselves_are_allowed(capi, ok):
    """on a machine without a GPU an allowed config fails at the device check, never as a bad argument"""
    try:
        capi.Gfr(**ok).close()
        status = capi.UZL_OK
    except capi.UzlError as e:
        status = e.status
    assert status in (capi.UZL_OK, capi.UZL_ERR_NO_DEVICE)


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        h = capi.Gfr()
        h.close()
        with pytest.raises(capi.UzlError) as e:
            capi.Gfr(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Gfr()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
