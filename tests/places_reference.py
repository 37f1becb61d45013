"""Plain-Python restatement of the uzl_places_* contract (include/uzl_mi355x.h), written from the semantics of FastLshTable /
FastLshSet / LshSetRecognizer (place_recognition/src/lsh_set_recognizer.cpp:46-305) behind the filters of PlaceRecognizer
(place_recognizer.cpp:71-215), independently of the CPU checker's and the HIP code's data structures.

One dict per table, one table per byte offset 0, kw, 2 kw, ... < 32 - kw + 1; key = kw descriptor bytes read little-endian;
value = list of place indices, one entry per descriptor row that produced the key.  Descriptor bytes from 32 up are never read.

  search_and_add  rows > min_rows_to_add: per (row, table) count the key's list, then push - only for keys with more than 3 kw set
                  bits (matchAndAdd); otherwise count only, every key (match).  The new place's own slot of the counts therefore
                  holds its self-collisions.
  add             rows > min_rows_to_add: push every key, unfiltered.
  search          count every key, unfiltered; an empty handle reports nothing and keeps the counts of the call before.
  remove          erase every occurrence of the place under the rows' keys; an unknown, negative or removed id is a no-op.
  finish          similarity = float32(count) / float32(tables), kept when >= T, ordered (similarity descending, index ascending);
                  then in order: dropped unless alive and |stamp difference| * 1e-9 > min_time_gap (integer difference first); each
                  survivor counts towards k_nearest_neighbors (the walk stops after the survivor that makes the count reach k, so
                  k <= 0 behaves as k = 1) and is reported unless (neighbour, query place) was reported before.  A pair is
                  registered even when it falls beyond the caller's cap."""
import numpy as np


def num_tables(key_width):
    return len(range(0, 32 - key_width + 1, key_width))


def keys_of(desc, key_width):
    """(rows x bytes) u8 -> list per row of the tables' integer keys"""
    d = np.ascontiguousarray(desc, np.uint8)
    if d.ndim != 2 or d.shape[0] == 0:
        return []
    if d.shape[1] < 32:
        raise ValueError("descriptors must be at least 32 bytes")
    starts = range(0, 32 - key_width + 1, key_width)
    return [[int.from_bytes(row[s:s + key_width], "little") for s in starts] for row in (r.tobytes() for r in d)]


def popcount(key):
    return bin(key).count("1")


class PlacesReference:
    def __init__(self, key_width=8, min_rows_to_add=150, T=10.0, k_nearest_neighbors=10, min_time_gap=5.0):
        if not 1 <= key_width <= 8:
            raise ValueError("key_width must be 1..8")
        if min_time_gap < 0:
            raise ValueError("min_time_gap must not be negative")
        self.kw, self.min_rows, self.T, self.k, self.gap = int(key_width), int(min_rows_to_add), float(T), int(k_nearest_neighbors), float(min_time_gap)
        self.nt = num_tables(self.kw)
        self.tables = [dict() for _ in range(self.nt)]
        self.stamp, self.alive = [], []
        self.checked = set()
        self.counts = np.zeros(0, np.int64)      # of the last search / search_and_add
        self.last_n = 0                          # full number of neighbours of the last search / search_and_add (cap or not)
        self.kept = self.skipped = 0             # keys that passed / failed matchAndAdd's popcount rule so far

    def num_tables(self):
        return self.nt

    def count(self):
        return len(self.stamp)

    def last_counts(self):
        return self.counts.copy()

    def _match(self, keys, counts):
        for row in keys:
            for t, k in enumerate(row):
                for p in self.tables[t].get(k, ()):
                    counts[p] += 1

    def _finish(self, counts, stamp_q, id_q, cap):
        """-> the reported neighbours, at most cap of them; last_n = their full number"""
        self.counts = np.array(counts, np.int64)
        m = []
        for i, c in enumerate(counts):
            if c > 0:
                sim = np.float32(c) / np.float32(self.nt)
                if float(sim) >= self.T:
                    m.append((-float(sim), i))
        m.sort()
        out, pr = [], 0
        for _, nb in m:
            if nb >= len(self.alive) or not self.alive[nb]:
                continue
            if not abs((self.stamp[nb] - int(stamp_q)) * 1e-9) > self.gap:
                continue
            pr += 1
            if (nb, id_q) not in self.checked:
                self.checked.add((nb, id_q))
                out.append(nb)
            if pr >= self.k:
                break
        self.last_n = len(out)
        return np.array(out[:max(cap, 0)], np.int32)

    def search_and_add(self, desc, stamp_ns, cap=64):
        """-> (neighbours, place index)"""
        keys = keys_of(desc, self.kw)
        pid = len(self.stamp)
        counts = [0] * (pid + 1)
        if len(keys) > self.min_rows:
            for row in keys:
                for t, k in enumerate(row):
                    if popcount(k) > 3 * self.kw:
                        self.kept += 1
                        lst = self.tables[t].setdefault(k, [])
                        for p in lst:
                            counts[p] += 1
                        lst.append(pid)
                    else:
                        self.skipped += 1
        else:
            self._match(keys, counts)
        self.stamp.append(int(stamp_ns)); self.alive.append(True)
        return self._finish(counts, stamp_ns, pid, cap), pid

    def add(self, desc, stamp_ns):
        keys = keys_of(desc, self.kw)
        pid = len(self.stamp)
        if len(keys) > self.min_rows:
            for row in keys:
                for t, k in enumerate(row):
                    self.tables[t].setdefault(k, []).append(pid)
        self.stamp.append(int(stamp_ns)); self.alive.append(True)
        return pid

    def search(self, desc, stamp_ns, query_place=-1, cap=64):
        self.last_n = 0
        if not self.stamp:
            return np.zeros(0, np.int32)
        counts = [0] * len(self.stamp)
        self._match(keys_of(desc, self.kw), counts)
        return self._finish(counts, stamp_ns, int(query_place), cap)

    def remove(self, place, desc):
        if not 0 <= place < len(self.alive) or not self.alive[place]:
            return
        for row in keys_of(desc, self.kw):
            for t, k in enumerate(row):
                lst = self.tables[t].get(k)
                if lst is not None:
                    lst[:] = [p for p in lst if p != place]
                    if not lst:
                        del self.tables[t][k]
        self.alive[place] = False
