#!/usr/bin/env python3
"""Diagnostic: uzl_gist_* timings.  Single-query latency (uzl_gist_search, host wall clock per call: upload, one launch, read-back,
filters) at 1k / 20k / 50k indexed places, and the rate of a 20k-node batched replay (uzl_gist_search_and_add_batch on an empty
handle: a triangle of ~2e8 distance pairs).  Kernel-only times: run under rocprofv3 --kernel-trace --stats (gist_knn_kernel)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from uzliti_slam_amd import capi    # noqa: E402

S = 10**9


def descriptors(rng, n, nbytes=32):
    """a camera run: each frame a few bits off the previous one, now and then a fresh view or a revisit"""
    d = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    for i in range(1, n):
        if rng.random() < 0.9:
            d[i] = d[i - 1] if rng.random() < 0.85 else d[rng.integers(0, i)]
            b = rng.integers(0, 8 * nbytes, 3)
            d[i, b // 8] ^= (1 << (b % 8)).astype(np.uint8)
    return d


def main():
    rng = np.random.default_rng(0)
    all_d = descriptors(rng, 50000)
    stamps = np.arange(50000, dtype=np.int64) * (S // 2)
    for n in (1000, 20000, 50000):
        g = capi.Gist()
        g.add_batch(all_d[:n], stamps[:n])
        q = descriptors(rng, 300)
        for i in range(20):
            g.search(q[i], 0)
        ts = []
        for i in range(300):
            t0 = time.perf_counter(); g.search(q[i], 10**6 * S); ts.append(time.perf_counter() - t0)
        ts.sort()
        print("single search, %6d places: median %.1f us, p10 %.1f us, p90 %.1f us (host wall per call)"
              % (n, 1e6 * ts[150], 1e6 * ts[30], 1e6 * ts[270]), flush=True)
        g.close()
    for rep in range(3):
        g = capi.Gist()
        t0 = time.perf_counter()
        lists, first, total = g.search_and_add_batch(all_d[:20000], stamps[:20000])
        dt = time.perf_counter() - t0
        print("batched replay, 20000 nodes: %.1f ms -> %.0f queries/s (%d neighbours reported)" % (1e3 * dt, 20000 / dt, total), flush=True)
        g.close()


if __name__ == "__main__":
    main()
