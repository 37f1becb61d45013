"""Which passes of the device-resident LM loop send their PCG init in the head's launch (lm_init_rides, csrc/pgo_lm_pass.hpp), on the
CPU through uzl_debug_lm_pass_plan of the diagnostic library: a pass that starts a trial, of one graph launched by value, without a
synchronous set-up (it rewrites the geometry the init reads, behind the head) and not on a Schur-reduced system (its right-hand side
is made behind the head).  A rebuild of the other hierarchy copy does not matter."""
import itertools
import os

import pytest

from uzliti_slam_amd import capi

SETUP, REBUILD = 1, 2          # LmPassFlags


@pytest.fixture(autouse=True)
def _needs_the_diagnostic_library():
    if not os.path.exists(capi.DIAG_LIB_PATH):
        pytest.skip("diagnostic library not built")


def rides(flags=0, any_start=True, pcg_args_pass=True, reduced=False):
    return capi.lm_pass_plan("init_rides", flags=flags, any_start=any_start, pcg_args_pass=pcg_args_pass, reduced=reduced)


def test_a_starting_pass_of_one_small_graph_rides():
    assert rides() is True and rides(flags=REBUILD) is True


def test_a_synchronous_setup_keeps_the_separate_init():
    assert rides(flags=SETUP) is False and rides(flags=SETUP | REBUILD) is False


def test_a_continuation_pass_has_neither():
    assert rides(any_start=False) is False


def test_batches_large_graphs_and_reduced_systems_keep_it():
    assert rides(pcg_args_pass=False) is False and rides(reduced=True) is False


def test_every_combination():
    for flags, start, args, red in itertools.product(range(4), (False, True), (False, True), (False, True)):
        assert rides(flags, start, args, red) == (start and not (flags & SETUP) and args and not red)
