"""The chunk split of the image stager (csrc/image_stager.hpp: plan_chunks), which uzl_laserline_extract and uzl_depthfilter_refine
use with 64 MB and 8192 images: items are taken in order while the chunk has fewer than max_items, and an item joins the chunk if
it is the chunk's first or the chunk's bytes stay within max_bytes.  Host arithmetic of the diagnostic build (uzl_debug_plan_chunks):
runs without a device."""
import ctypes as C

import numpy as np

from uzliti_slam_amd import capi

MAX_BYTES, MAX_ITEMS = 100, 4


def plan(sizes, max_bytes=MAX_BYTES, max_items=MAX_ITEMS):
    """the chunks as (first, end) pairs"""
    L = capi.diag_lib()
    b = np.asarray(sizes, np.int64)
    first = np.full(len(b) + 1, -7, np.int32)
    n = L.uzl_debug_plan_chunks(C.c_int32(len(b)), b.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(max_bytes), C.c_int32(max_items),
                                first.ctypes.data_as(C.POINTER(C.c_int32)))
    assert 0 <= n <= len(b), n
    assert (first[n + 1:] == -7).all()                                      # nothing written past the boundaries
    return [(int(first[k]), int(first[k + 1])) for k in range(n)]


def rule(sizes, max_bytes, max_items):
    """the rule, restated"""
    chunks, i0 = [], 0
    while i0 < len(sizes):
        i1, total = i0, 0
        while i1 < len(sizes) and i1 - i0 < max_items and (i1 == i0 or total + sizes[i1] <= max_bytes):
            total += sizes[i1]; i1 += 1
        chunks.append((i0, i1)); i0 = i1
    return chunks


def test_no_items_and_everything_fits():
    assert plan([]) == []
    assert plan([10]) == [(0, 1)]
    assert plan([10, 20, 30]) == [(0, 3)]


def test_exactly_max_bytes_stays_together_and_one_byte_more_splits():
    assert plan([40, 30, 30]) == [(0, 3)]
    assert plan([40, 30, 31]) == [(0, 2), (2, 3)]
    assert plan([100]) == [(0, 1)]
    assert plan([100, 1]) == [(0, 1), (1, 2)]
    assert plan([50, 50, 50, 50]) == [(0, 2), (2, 4)]


def test_an_item_larger_than_max_bytes_is_a_chunk_of_its_own():
    assert plan([101]) == [(0, 1)]
    assert plan([500, 10, 10]) == [(0, 1), (1, 3)]                          # at the head
    assert plan([10, 10, 500, 10, 10]) == [(0, 2), (2, 3), (3, 5)]          # in the middle
    assert plan([10, 10, 500]) == [(0, 2), (2, 3)]                          # at the tail
    assert plan([500, 500]) == [(0, 1), (1, 2)]
    assert plan([500, 0]) == [(0, 1), (1, 2)]                               # nothing joins a chunk that is over the limit already


def test_zero_byte_items_join_the_open_chunk_up_to_max_items():
    assert plan([0, 0, 0]) == [(0, 3)]
    assert plan([100, 0, 0]) == [(0, 3)]
    assert plan([0, 0, 0, 0, 0, 0]) == [(0, 4), (4, 6)]
    assert plan([60, 0, 40, 0, 1]) == [(0, 4), (4, 5)]
    assert plan([60, 0, 41, 0]) == [(0, 2), (2, 4)]


def test_the_max_items_cap():
    assert plan([1] * 4) == [(0, 4)]
    assert plan([1] * 5) == [(0, 4), (4, 5)]
    assert plan([1] * 9) == [(0, 4), (4, 8), (8, 9)]
    assert plan([1] * 3, max_items=1) == [(0, 1), (1, 2), (2, 3)]
    assert plan([30] * 7, max_items=8) == [(0, 3), (3, 6), (6, 7)]          # the byte limit first
    assert plan([7, 8], max_bytes=0) == [(0, 1), (1, 2)]
    assert plan([0, 0, 7], max_bytes=0) == [(0, 2), (2, 3)]


def test_random_lists_against_the_restated_rule():
    rng = np.random.default_rng(20)
    for case in range(400):
        n = int(rng.integers(0, 40))
        max_bytes = int(rng.integers(0, 200))
        max_items = int(rng.integers(1, 9))
        sizes = rng.integers(0, [1, 30, 120, 400][case % 4] + 1, n)
        sizes[rng.random(n) < 0.15] = 0
        sizes = [int(v) for v in sizes]
        chunks = plan(sizes, max_bytes, max_items)
        assert chunks == rule(sizes, max_bytes, max_items), (sizes, max_bytes, max_items)
        # contiguous, non-empty, covering 0..n
        assert all(a < b for a, b in chunks) and [a for a, _ in chunks] + [n] == [0] + [b for _, b in chunks]
        for a, b in chunks:
            assert b - a <= max_items
            assert b - a == 1 or sum(sizes[a:b]) <= max_bytes, (sizes, max_bytes, max_items, (a, b))


def test_arguments_the_rule_does_not_take():
    L = capi.diag_lib()
    b = np.array([1, 2], np.int64)
    out = np.zeros(3, np.int32)
    bp, op = b.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.uzl_debug_plan_chunks(C.c_int32(2), bp, C.c_int64(10), C.c_int32(0), op) == -1      # a chunk takes at least one item
    assert L.uzl_debug_plan_chunks(C.c_int32(-1), bp, C.c_int64(10), C.c_int32(4), op) == -1
    assert L.uzl_debug_plan_chunks(C.c_int32(2), None, C.c_int64(10), C.c_int32(4), op) == -1
    assert L.uzl_debug_plan_chunks(C.c_int32(2), bp, C.c_int64(10), C.c_int32(4), None) == -1
