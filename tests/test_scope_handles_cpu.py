"""CPU tests (no GPU needed): uzl_scope_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp: HandleBase,
UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_gfr_handles_cpu.py.  What needs a handle runs on
the device when there is one and is skipped over inside the test otherwise, so the tests pass with or without a GPU."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

EXPORTS = ["uzl_scope_cfg_default", "uzl_scope_create", "uzl_scope_destroy", "uzl_scope_last_error", "uzl_scope_set_graph", "uzl_scope_add",
           "uzl_scope_set_poses", "uzl_scope_poses_from_pgo", "uzl_scope_set_valid", "uzl_scope_set_uncertainty", "uzl_scope_reevaluate",
           "uzl_scope_uncertainty", "uzl_scope_distance", "uzl_scope_request", "uzl_scope_select", "uzl_scope_stats", "uzl_scope_lds_nodes"]


def test_exports_present(capi):
    L = capi.lib()
    for name in EXPORTS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set(re.findall(r"\b(uzl_scope_[a-z0-9_]+)\b", out))
    assert found == set(EXPORTS)                     # nothing of the handle's internals (the solver's pose accessor) leaks out


def test_null_handle(capi):
    L = capi.lib()
    n = C.c_int32(); d = C.c_double(); r = C.c_int64()
    assert L.uzl_scope_last_error(None) == b"null handle"
    assert L.uzl_scope_destroy(None) is None
    assert L.uzl_scope_cfg_default(None) is None
    assert L.uzl_scope_create(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_graph(None, 0, None, None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_add(None, 0, None, None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_poses(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_poses_from_pgo(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_valid(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_uncertainty(None, 0, C.c_double(1.0)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_reevaluate(None, -1, C.byref(n), C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_uncertainty(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_distance(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_request(None, 0, C.byref(d), 0, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_select(None, None, C.c_double(1.0), 0, None, 0, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_stats(None, C.byref(r), C.byref(r), C.byref(n)) == capi.UZL_ERR_BAD_ARG


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_scope" in capi._MORE_HANDLES and "uzl_scope" not in capi._HANDLES


def test_defaults_and_the_mirrored_bound(capi):
    c = capi.ScopeCfg()
    capi.lib().uzl_scope_cfg_default(C.byref(c))
    assert (c.scope_size_min, c.scope_size_factor, c.out_margin, c.device, c._pad) == (8.0, 0.1, 4.0, 0, 0)
    assert C.sizeof(capi.ScopeCfg) == 32
    assert (capi.ScopeCfg.scope_size_min.offset, capi.ScopeCfg.scope_size_factor.offset, capi.ScopeCfg.out_margin.offset,
            capi.ScopeCfg.device.offset) == (0, 8, 16, 24)
    capi.lib().uzl_scope_lds_nodes.restype = C.c_int32
    assert capi.lib().uzl_scope_lds_nodes() == capi.SCOPE_LDS_NODES
    # 8 B of distance per node and two frontier bitmaps fit the 160 KiB of a CU
    assert capi.SCOPE_LDS_NODES * 8 + 2 * capi.SCOPE_LDS_NODES // 8 <= 160 * 1024


BAD = [dict(scope_size_min=math.nan), dict(scope_size_factor=math.nan), dict(out_margin=math.nan)]


@pytest.mark.parametrize("bad", BAD, ids=[k for b in BAD for k in b])
def test_argument_errors_come_before_the_device_check(capi, bad):
    with pytest.raises(capi.UzlError) as e:
        capi.Scope(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        capi.Scope().close()
        with pytest.raises(capi.UzlError) as e:
            capi.Scope(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Scope()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
    with pytest.raises(capi.UzlError) as e:
        capi.Scope(device=-1)
    assert e.value.status == capi.UZL_ERR_NO_DEVICE


def test_lifecycle_and_argument_errors_on_a_handle(capi):
    """with a device: NULL arguments, a cap too small, nodes out of range, close twice; the handle stays usable after every refusal"""
    if capi.device_count() <= 0:
        with pytest.raises(capi.UzlError):
            capi.Scope()
        return
    import scope_scenes as S
    L = capi.lib()
    sc = S.two_components()
    h = capi.Scope()
    n = C.c_int32(-5); st = C.c_int32(-5); d = C.c_double()
    assert L.uzl_scope_reevaluate(h._h, -1, C.byref(st), C.byref(n)) == capi.UZL_OK and (st.value, n.value) == (-1, 0)      # empty graph
    assert L.uzl_scope_set_graph(h._h, 2, None, None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_graph(h._h, 0, None, None, 1, None) == capi.UZL_ERR_BAD_ARG
    bad = S.edges_of([(0, 6)])
    with pytest.raises(capi.UzlError) as e:
        h.set_graph(sc["poses"], sc["unc"], bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG and "outside" in str(e.value)
    h.set_graph(sc["poses"], sc["unc"], sc["edges"])
    assert L.uzl_scope_distance(h._h, 6, np.zeros(6).ctypes.data_as(capi.c_f64p)) == capi.UZL_ERR_STATE                   # no pass yet
    assert h.reevaluate(6) == (-1, 0)                                      # existsNode == false: succeeds, nothing changes
    assert np.array_equal(h.uncertainty(), sc["unc"])
    assert h.reevaluate(5) == (3, 3)
    buf = np.zeros(6)
    assert L.uzl_scope_uncertainty(h._h, 5, buf.ctypes.data_as(capi.c_f64p)) == capi.UZL_ERR_BAD_ARG                      # cap too small
    assert L.uzl_scope_distance(h._h, 5, buf.ctypes.data_as(capi.c_f64p)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_uncertainty(h._h, 6, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_uncertainty(h._h, 6, buf.ctypes.data_as(capi.c_f64p)) == 6
    assert L.uzl_scope_request(h._h, 0, C.byref(d), 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_request(h._h, 0, C.byref(d), 4, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_request(h._h, 6, C.byref(d), 0, None, C.byref(n)) == capi.UZL_ERR_NOT_FOUND
    assert L.uzl_scope_request(h._h, -1, C.byref(d), 0, None, C.byref(n)) == capi.UZL_ERR_NOT_FOUND
    assert L.uzl_scope_request(h._h, 0, None, 0, None, C.byref(n)) == capi.UZL_OK and n.value == 0                        # all within 12 m
    assert L.uzl_scope_select(h._h, None, C.c_double(1.0), 0, None, 0, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_select(h._h, np.zeros(3).ctypes.data_as(capi.c_f64p), C.c_double(1.0), 2, None, 0, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_uncertainty(h._h, 6, C.c_double(1.0)) == capi.UZL_ERR_NOT_FOUND
    assert L.uzl_scope_set_poses(h._h, 5, sc["poses"].ctypes.data_as(capi.c_f64p)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_poses(h._h, 6, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_poses_from_pgo(h._h, None) == capi.UZL_ERR_BAD_ARG
    one = np.array([4], np.int32); flag = np.array([1], np.uint8)
    assert L.uzl_scope_set_valid(h._h, 1, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scope_set_valid(h._h, 1, one.ctypes.data_as(capi.c_i32p), flag.ctypes.data_as(capi.c_u8p)) == capi.UZL_ERR_BAD_ARG
    assert b"no such edge" in L.uzl_scope_last_error(h._h)
    assert h.reevaluate(5) == (3, 3)                                       # still usable
    assert h.stats()["in_lds"] == 1
    h.close()
    h.close()
