"""CPU tests (no GPU needed): the lifecycle and error path every uzl_* handle shares (uzl_common.hpp: HandleBase, UZL_GUARD_*,
last_error_of, check_device; capi._Handle).  Nothing here creates a handle on a device, so they pass with or without one."""
import ctypes

import pytest

PREFIXES = ("uzl_match", "uzl_pgo", "uzl_pgo_batch", "uzl_filter", "uzl_gate", "uzl_radius", "uzl_places", "uzl_gist")

# one guarded entry point per handle type, called with a NULL handle and arguments that are otherwise harmless
GUARDED = {
    "uzl_match": ("uzl_match_collect", (None, None, None, None, None, None)),
    "uzl_pgo": ("uzl_pgo_reset", (None,)),
    "uzl_pgo_batch": ("uzl_pgo_batch_optimize", (None, 0, None, None)),
    "uzl_filter": ("uzl_filter_set_sensors", (None, 0, None)),
    "uzl_gate": ("uzl_gate_set_graph", (None, 0, None, None, 0, None)),
    "uzl_radius": ("uzl_radius_set_nodes", (None, 0, None, None)),
    "uzl_places": ("uzl_places_remove", (None, 0, None, 0, 0)),
    "uzl_gist": ("uzl_gist_remove", (None, 0)),
}


@pytest.mark.parametrize("prefix", PREFIXES)
def test_null_handle(capi, prefix):
    L = capi.lib()
    assert getattr(L, prefix + "_last_error")(None) == b"null handle"
    assert getattr(L, prefix + "_destroy")(None) is None
    fn, args = GUARDED[prefix]
    assert getattr(L, fn)(*args) == capi.UZL_ERR_BAD_ARG


def test_every_handle_type_is_covered(capi):
    assert set(GUARDED) == set(PREFIXES) == set(capi._HANDLES)


@pytest.mark.parametrize("make", [
    lambda capi: capi.Places(key_width=0),
    lambda capi: capi.Gist(k_nearest_neighbors=-1),
    lambda capi: capi.Filter(max_cluster_size=0),
    lambda capi: capi.PgoBatch(0),
], ids=["places_key_width", "gist_k", "filter_max_cluster_size", "batch_n_graphs"])
def test_argument_errors_come_before_the_device_check(capi, make):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        make(capi)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_create_without_an_out_pointer(capi):
    L = capi.lib()
    for p in PREFIXES:
        args = (None, ctypes.c_int32(1), None) if p == "uzl_pgo_batch" else (None, None)
        assert getattr(L, p + "_create")(*args) == capi.UZL_ERR_BAD_ARG, p
