"""Pure-NumPy restatement of GlobalFeatureRepositoryRecognizer (place_recognition/src/global_feature_repository_recognizer.cpp)
over GlobalFeatureRepository (global_feature_repository.cpp) behind PlaceRecognizer (place_recognizer.cpp:71-180), with the exact
nearest-feature search that include/uzl_mi355x.h makes the contract in place of FLANN's LSH index.  Written from the reference and
the header's contract, independently of the HIP host code.

A match: a type change clears the repository; every row finds min (Hamming distance, feature index) over the repository as it stood
before the node and is matched iff distance < max_distance; a matched row votes once per entry of its feature's links; candidates
are the places with votes > 0 and >= T by (votes descending, place ascending); then PlaceRecognizer's filters.  Integration: an
unmatched row with popcount > 3 * bytes becomes a feature linked to this place, a matched row appends this place to its feature.

`counters` records what the sequence met, so that a test can assert its data reached the edge cases."""
import numpy as np


def _words(rows, nbytes):
    """rows (n x nbytes) u8 -> (n x ceil(nbytes / 8)) u64, zero-padded (padding changes neither distances nor popcounts)"""
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, nbytes)
    w = (nbytes + 7) // 8
    pad = np.zeros((rows.shape[0], 8 * w), np.uint8)
    pad[:, :nbytes] = rows
    return pad.view(np.uint64)


def nearest(store_words, row_words, chunk=64):
    """per row: (feature, distance) of min (distance, feature) over the store; (-1, -1) for an empty store"""
    n = row_words.shape[0]
    if store_words.shape[0] == 0:
        return np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    ft = np.zeros(n, np.int64); di = np.zeros(n, np.int64)
    for r0 in range(0, n, chunk):
        x = np.bitwise_xor(row_words[r0:r0 + chunk, None, :], store_words[None, :, :])
        d = np.bitwise_count(x).sum(axis=2, dtype=np.int64)
        f = d.argmin(axis=1)                                       # the first minimum: ties go to the lower index
        ft[r0:r0 + chunk] = f
        di[r0:r0 + chunk] = d[np.arange(len(f)), f]
    return ft, di


class GfrReference:
    def __init__(self, T=10.0, k_nearest_neighbors=10, max_distance=40, min_time_gap=5.0, **_):
        self.T, self.k, self.max_distance, self.min_time_gap = float(T), int(k_nearest_neighbors), int(max_distance), float(min_time_gap)
        self.stamp, self.alive = [], []       # per place index
        self.checked = set()
        self.type = -1
        self.bytes = None                     # of the stored features
        self._store = np.zeros((0, 1), np.uint64)
        self.F = 0
        self.links = []                       # per feature: place indices in insertion order (= ascending)
        self.last_matches = (np.zeros(0, np.int32), np.zeros(0, np.int32))
        self.last_votes = np.zeros(0, np.int32)
        self.counters = dict(at_max_minus_1=0, at_max=0, popcount_drops=0, duplicate_links=0, vote_ties=0, neighbours=0)

    # ---- GlobalFeatureRepository
    def _clear(self):
        self.links, self.F, self.bytes = [], 0, None
        self._store = np.zeros((0, 1), np.uint64)

    def _check(self, desc, feature_type):
        """the argument errors of a call, before anything changes; returns the rows or None"""
        if desc is None:
            return None
        d = np.asarray(desc, np.uint8)
        rows = d.shape[0]
        if rows > 4096:
            raise ValueError("rows must be 0-4096")
        if rows == 0:
            return None
        nbytes = d.reshape(rows, -1).shape[1]
        if not 1 <= nbytes <= 64:
            raise ValueError("descriptor length must be 1-64 bytes")
        if feature_type == self.type and self.F > 0 and nbytes != self.bytes:
            raise ValueError("descriptor length differs from the stored features")
        return d.reshape(rows, nbytes)

    def _match(self, d, feature_type, votes):
        """steps a-d; returns (matched feature per row or -1, candidates best first)"""
        if feature_type != self.type:
            self.type = feature_type
            self._clear()
        rows, nbytes = d.shape
        w = _words(d, nbytes)
        ft, di = nearest(self._store[:self.F], w) if self.F else nearest(np.zeros((0, w.shape[1]), np.uint64), w)
        matched = (ft >= 0) & (di < self.max_distance)
        self.counters["at_max_minus_1"] += int(np.sum(di == self.max_distance - 1))
        self.counters["at_max"] += int(np.sum((ft >= 0) & (di == self.max_distance)))
        m = np.where(matched, ft, -1)
        self.last_matches = (m.astype(np.int32), di.astype(np.int32))
        cand = []
        if votes:
            v = np.zeros(len(self.stamp) + 1, np.int64)
            for f in m[m >= 0]:
                np.add.at(v, self.links[f], 1)
            self.last_votes = v.astype(np.int32)
            cand = candidates(v, self.T)
            vs = [int(v[p]) for p in cand]
            self.counters["vote_ties"] += len(vs) - len(set(vs))
        return m, cand

    def _integrate(self, d, m, place):
        rows, nbytes = d.shape
        w = _words(d, nbytes)
        pop = np.bitwise_count(w).sum(axis=1)
        seen = set()
        for i in range(rows):
            if m[i] < 0:
                if pop[i] > 3 * nbytes:
                    if self.F == 0:
                        self.bytes = nbytes
                        self._store = np.zeros((256, w.shape[1]), np.uint64)
                    if self.F == self._store.shape[0]:
                        self._store = np.concatenate([self._store, np.zeros_like(self._store)])
                    self._store[self.F] = w[i]
                    self.links.append([place])
                    self.F += 1
                else:
                    self.counters["popcount_drops"] += 1
            else:
                f = int(m[i])
                self.counters["duplicate_links"] += f in seen
                seen.add(f)
                self.links[f].append(place)

    # ---- PlaceRecognizer's filters (place_recognizer.cpp:87-114, 157-180)
    def _filter(self, places, stamp_q, id_q):
        res, pr = [], 0
        for nb in places:
            nb = int(nb)
            if not (0 <= nb < len(self.alive)) or not self.alive[nb]:
                continue
            if not abs((self.stamp[nb] - int(stamp_q)) * 1e-9) > self.min_time_gap:
                continue
            pr += 1
            if (nb, id_q) not in self.checked:
                self.checked.add((nb, id_q))
                res.append(nb)
            if pr >= self.k:                  # tested after the neighbour is taken: k = 0 lets one through
                break
        self.counters["neighbours"] += len(res)
        return np.array(res, np.int32)

    def _commit(self, stamp_ns):
        self.stamp.append(int(stamp_ns)); self.alive.append(True)
        return len(self.stamp) - 1

    # ---- public
    def search_and_add(self, desc, stamp_ns, feature_type=2):
        d = self._check(desc, feature_type)
        place = len(self.stamp)
        cand = []
        if d is not None:
            m, cand = self._match(d, feature_type, True)
            self._integrate(d, m, place)
        self._commit(stamp_ns)
        return self._filter(cand, stamp_ns, place), place

    def add(self, desc, stamp_ns, feature_type=2):
        d = self._check(desc, feature_type)
        place = len(self.stamp)
        if d is not None:
            m, _ = self._match(d, feature_type, False)      # no votes: see the header on addPlaceImpl
            self._integrate(d, m, place)
        return self._commit(stamp_ns)

    def search(self, desc, stamp_ns, feature_type=2, query_place=-1):
        d = self._check(desc, feature_type)
        if not any(self.alive) or d is None:
            return np.zeros(0, np.int32)
        _, cand = self._match(d, feature_type, True)
        return self._filter(cand, stamp_ns, int(query_place))

    def remove(self, place):
        if not 0 <= place < len(self.alive) or not self.alive[place]:
            raise KeyError(place)
        self.alive[place] = False

    def count(self):
        return len(self.stamp)

    def feature_count(self):
        return self.F

    def link_count(self):
        return sum(len(x) for x in self.links)

    def get_feature(self, f):
        return self._store[f].view(np.uint8)[:self.bytes].copy(), np.array(self.links[f], np.int32)


def candidates(votes, T):
    """step d: places with votes > 0 and votes >= T, by (votes descending, place ascending)"""
    p = np.flatnonzero((votes > 0) & (votes >= T))
    return [int(x) for x in p[np.lexsort((p, -votes[p]))]]


# ---- plain-loop forms of steps b-d (CPU cross-check of the vectorised ones)
def brute_nearest(features, row):
    """features = list of byte sequences; (feature, distance) of min (distance, index), (-1, -1) for none"""
    best = (-1, -1)
    for f, feat in enumerate(features):
        dist = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(row, feat))
        if best[0] < 0 or dist < best[1]:
            best = (f, dist)
    return best


def brute_votes(features, links, rows, max_distance, n_places):
    votes = [0] * (n_places + 1)
    matches = []
    for row in rows:
        f, dist = brute_nearest(features, row)
        ok = f >= 0 and dist < max_distance
        matches.append((f if ok else -1, dist))
        if ok:
            for p in links[f]:
                votes[p] += 1
    return matches, votes


def brute_candidates(votes, T):
    c = [(-v, p) for p, v in enumerate(votes) if v > 0 and v >= T]
    c.sort()
    return [p for _, p in c]
