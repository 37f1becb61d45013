"""Pure-NumPy restatement of BinaryGistRecognizer (place_recognition/src/binary_gist_recognizer.cpp) behind PlaceRecognizer
(place_recognizer.cpp:71-180), with the exact k-NN that include/uzl_mi355x.h makes the contract in place of FLANN's LSH index.
Written from the reference and the header's contract, independently of the HIP host code.

A search: every live indexed place, sorted by (Hamming distance, place index); the first k; of those the ones with distance <= T;
then, for each in order, the time gap |dt| > min_time_gap, the k cut and the reported-once filter on (neighbour, query) pairs."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b):
    """Hamming distances between one descriptor a (bytes) and the rows of b (n x bytes)."""
    a = np.asarray(a, np.uint8).reshape(1, -1)
    b = np.asarray(b, np.uint8).reshape(-1, a.shape[1])
    return _POP[np.bitwise_xor(a, b)].sum(axis=1)


class GistReference:
    def __init__(self, T=10.0, k_nearest_neighbors=10, min_time_gap=5.0):
        self.T, self.k, self.min_time_gap = float(T), int(k_nearest_neighbors), float(min_time_gap)
        self.stamp = []          # per place index, ns
        self.alive = []          # in place_id_map_
        self.desc = []           # per place: bytes or None (no GIST sensor)
        self.bytes = None
        self.checked = set()
        self.last_knn = (np.zeros(0, np.int32), np.zeros(0, np.int32))

    # ---- the recognizer (impl) part
    def _check_len(self, desc):
        n = len(desc)
        if not 1 <= n <= 256:
            raise ValueError("descriptor length must be 1-256 bytes")
        if self.bytes is not None and n != self.bytes:
            raise ValueError("descriptor length differs from the first indexed one")

    def _knn(self, desc):
        """the impl's result: k nearest live indexed places within T, nearest first (place, distance)"""
        idx = [p for p, d in enumerate(self.desc) if d is not None and self.alive[p]]
        if desc is None or not idx or self.k <= 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        dist = hamming(desc, np.stack([self.desc[p] for p in idx]))
        order = np.lexsort((np.array(idx), dist))[:self.k]
        pl = np.array(idx, np.int64)[order]
        di = dist[order]
        keep = di <= self.T
        return pl[keep].astype(np.int32), di[keep].astype(np.int32)

    def _index(self, desc, stamp_ns):
        if desc is not None:
            desc = np.asarray(desc, np.uint8).reshape(-1).copy()
            if self.bytes is None:
                self.bytes = len(desc)
        self.desc.append(desc)
        self.stamp.append(int(stamp_ns))
        self.alive.append(True)
        return len(self.desc) - 1

    # ---- PlaceRecognizer's filters (place_recognizer.cpp:87-114)
    def _filter(self, places, stamp_q, id_q):
        res, pr = [], 0
        for nb in places:
            nb = int(nb)
            if not self.alive[nb]:
                continue
            if not abs((self.stamp[nb] - int(stamp_q)) * 1e-9) > self.min_time_gap:
                continue
            pr += 1
            if (nb, id_q) not in self.checked:
                self.checked.add((nb, id_q))
                res.append(nb)
            if pr >= self.k:
                break
        return np.array(res, np.int32)

    # ---- public
    def search_and_add(self, desc, stamp_ns):
        if desc is not None:
            self._check_len(desc)
        self.last_knn = self._knn(desc)
        pid = self._index(desc, stamp_ns)
        return self._filter(self.last_knn[0], stamp_ns, pid), pid

    def add(self, desc, stamp_ns):
        if desc is not None:
            self._check_len(desc)
        return self._index(desc, stamp_ns)

    def search(self, desc, stamp_ns, query_place=-1):
        if desc is not None:
            self._check_len(desc)
        self.last_knn = self._knn(desc) if self.desc else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        return self._filter(self.last_knn[0], stamp_ns, int(query_place))

    def remove(self, place):
        if not 0 <= place < len(self.alive) or not self.alive[place]:
            raise KeyError(place)
        self.alive[place] = False

    def count(self):
        return len(self.desc)


def brute_knn(store, alive, query, k, T):
    """loop form of the contract's steps 1-2 (CPU cross-check of GistReference._knn): store = list of bytes or None"""
    cand = []
    for p, d in enumerate(store):
        if d is None or not alive[p]:
            continue
        dist = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(query, d))
        cand.append((dist, p))
    cand.sort()
    return [(p, dist) for dist, p in cand[:max(k, 0)] if dist <= T]
