"""Wall time of uzl_scanmerge_run on 1,024 (keep, drop) pairs of 720-beam scans in one call, beside 1,024 single-pair calls of the
same pairs and the NumPy restatement's time per pair (tests/scanmerge_reference.py, on UZL_SCANMERGE_TIMING_REF pairs).  Wall time
= host clock around the call (packing the ctypes structs is outside it; the call checks, packs into pinned memory, copies, launches
and synchronises), median of UZL_SCANMERGE_TIMING_REPS calls after a warm-up that also makes the tables.  The same batch at 4,096
beams (256 pairs) shows the sort's growth.  Prints one JSON line per measurement; no threshold, not a test."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_SCANMERGE_TIMING_REPS", "7"))
REF = int(os.environ.get("UZL_SCANMERGE_TIMING_REF", "8"))


def median_ms(fn):
    wall = []
    for _ in range(REPS):
        t = time.perf_counter(); fn(); wall.append(time.perf_counter() - t)
    return 1e3 * float(np.median(wall))


def main():
    import scanmerge_reference as R
    import scanmerge_scenes as S
    from uzliti_slam_amd import capi
    h = capi.ScanMerge()
    for beams, n_pairs in ((720, 1024), (4096, 256)):
        rng = np.random.default_rng(beams)
        distinct = []
        for i in range(16):
            distinct.append((S.room(rng, beams, stamp_ns=1, displacement=S.generic(rng)), S.room(rng, beams, stamp_ns=2 + i % 2 * -2, displacement=S.generic(rng)),
                             S.generic(rng), S.generic(rng)))
        pairs = [distinct[i % 16] for i in range(n_pairs)]
        batch = h.pack_pairs(pairs)
        singles = [h.pack_pairs([p]) for p in pairs]
        h.run(batch)
        batch_ms = median_ms(lambda: h.run(batch))
        h.run(batch)
        got = [h.read(i) for i in range(16)]

        def one_by_one():
            for s in singles:
                h.run(s)

        single_ms = median_ms(one_by_one)
        t = time.perf_counter()
        want = [R.merge(*distinct[i]) for i in range(min(REF, 16))]
        ref_ms = 1e3 * (time.perf_counter() - t) / len(want)
        same = all(np.array_equal(g[0], w["ranges"]) and np.array_equal(g[1], w["intensities"]) and np.array_equal(g[2], w["center"])
                   for g, w in zip(got, want))
        in_mb = n_pairs * 4 * beams * 4 / 1e6
        print(json.dumps(dict(beams=beams, pairs=n_pairs, batch_ms=batch_ms, batch_us_per_pair=1e3 * batch_ms / n_pairs, single_calls_ms=single_ms,
                              single_us_per_pair=1e3 * single_ms / n_pairs, restatement_ms_per_pair=ref_ms, input_mb=in_mb, bit_equal=same,
                              reps=REPS)), flush=True)
    h.close()


if __name__ == "__main__":
    main()
