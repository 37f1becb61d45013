#!/usr/bin/env python3
"""Diagnostic: uzl_gfr_* timings.  Host wall clock per uzl_gfr_search_and_add (upload, up to four launches, one download, one wait,
filters) of a node of 300 rows x 64 bytes against a repository of about 1e4, 1e5 and 1e6 features, and the repository bytes that
one call streams (F x 64) over that time.  Two thirds of a node's rows are stored features with up to 12 bits flipped (they match and
link), one third are new (they become features), so the 230 calls of one size add 23,000 features to it.  Kernel-only times: run under rocprofv3 --kernel-trace --stats
(gfr_nearest_kernel)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from uzliti_slam_amd import capi    # noqa: E402

S = 10**9
ROWS, BYTES, FRESH = 300, 64, 100


def dense(rng, n):
    d = rng.integers(0, 256, (n, BYTES), dtype=np.uint8)
    d[:, :8] = 0xFF                                            # past the popcount rule whatever the rest holds
    return d


def node(rng, world):
    q = world[rng.integers(0, len(world), ROWS)].copy()
    for i in range(ROWS - FRESH):
        for b in rng.integers(64, 8 * BYTES, int(rng.integers(0, 13))):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    q[ROWS - FRESH:] = dense(rng, FRESH)
    return q


def main():
    rng = np.random.default_rng(0)
    for target in (10**4, 10**5, 10**6):
        world = dense(rng, target)
        g = capi.Gfr(initial_features=1 << 21)
        t0 = time.perf_counter()
        for f0 in range(0, target, 4096):
            g.add(world[f0:f0 + 4096], 0)
        fill = time.perf_counter() - t0
        nodes = [node(rng, world) for _ in range(230)]
        for i in range(30):
            g.search_and_add(nodes[i], (10 + i) * S)
        ts = []
        for i in range(30, 230):
            t0 = time.perf_counter(); nb, _ = g.search_and_add(nodes[i], (10 + i) * S); ts.append(time.perf_counter() - t0)
        ts.sort()
        F = g.feature_count()
        med = ts[len(ts) // 2]
        print("search_and_add, %d rows x %d bytes, F = %8d (filled in %.2f s): median %.1f us, p10 %.1f us, p90 %.1f us per call "
              "(host wall); repository %.1f MB / median = %.1f GB/s; %d links, last call reported %d neighbours"
              % (ROWS, BYTES, F, fill, 1e6 * med, 1e6 * ts[len(ts) // 10], 1e6 * ts[9 * len(ts) // 10], F * 64 / 1e6, F * 64 / med / 1e9,
                 g.link_count(), len(nb)), flush=True)
        g.close()


if __name__ == "__main__":
    main()
