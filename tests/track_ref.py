"""The detection-event contract (include/birdnet_hip.h, bn_track_*) stated in plain numpy / Python, independent of the product, one
(source, species) at a time.

For a row that is window k of source s, and species j with logit z:
    conf = oracle.sigmoid(z)
    with a prior (table, threshold, rerank) and the row's site: p = table[site][j]; a species that is not prior_ref.admitted is never
        a hit; conf = prior_ref.conf_prime(conf, p, rerank)
    hit  = conf >= enter_conf           (NaN is not a hit)
    an open event (hits > 0, last hit window `last`): misses = (k - last - 1) + (0 if hit else 1); misses > max_gap closes it; a closed
        event is emitted iff hits >= min_hits
    a hit opens (first = k, sum = 0, hits = 0, peak = conf, peak_window = k) or extends; then last = k, hits += 1, sum += conf (f32, in
        increasing k); conf > peak (strict) sets peak and peak_window
    mean = sum / float32(hits)
flush closes every open event of a source (or all) under the same min_hits rule; reset forgets a source's open events and last window.
The events of an update are sorted by (source, species, first_window)."""
import numpy as np

import prior_ref

EVENT_DTYPE = np.dtype([("source", np.int32), ("species", np.uint32), ("first_window", np.uint32), ("last_window", np.uint32),
                        ("hits", np.uint32), ("peak_window", np.uint32), ("peak_conf", np.float32), ("mean_conf", np.float32)])


def sort_events(ev):
    ev = np.asarray(ev, dtype=EVENT_DTYPE)
    return ev[np.lexsort((ev["first_window"], ev["species"], ev["source"]))]


def concat(parts):
    parts = [np.asarray(p, dtype=EVENT_DTYPE) for p in parts]
    return sort_events(np.concatenate(parts) if parts else np.zeros(0, dtype=EVENT_DTYPE))


class Tracker:
    def __init__(self, n_sources, n_species, enter_conf, min_hits=1, max_gap=0, prior=None):
        """prior: None or (table [n_sites, n_species], threshold, rerank)."""
        self.n_sources, self.n_species = n_sources, n_species
        self.enter, self.min_hits, self.max_gap, self.prior = np.float32(enter_conf), int(min_hits), int(max_gap), prior
        self.rec = {}                      # (source, species) -> [first, last, hits, peak_window, peak, sum]
        self.last_window = [-1] * n_sources

    def _close(self, s, j, out):
        first, last, hits, pw, peak, total = self.rec.pop((s, j))
        if hits >= self.min_hits:
            out.append((s, j, first, last, hits, pw, peak, np.float32(total) / np.float32(hits)))

    def _row(self, s, k, conf, prow, out):
        with np.errstate(invalid="ignore"):
            if prow is None:
                hit = conf >= self.enter
            else:
                _, thr, rerank = self.prior
                conf = prior_ref.conf_prime(conf, prow, rerank)
                hit = prior_ref.admitted(prow, thr) & (conf >= self.enter)
        touched = set(np.nonzero(hit)[0].tolist()) | {j for (ss, j) in self.rec if ss == s}
        for j in sorted(touched):
            h = bool(hit[j])
            if (s, j) in self.rec:
                last = self.rec[(s, j)][1]
                if (k - last - 1) + (0 if h else 1) > self.max_gap:
                    self._close(s, j, out)
            if h:
                c = np.float32(conf[j])
                r = self.rec.setdefault((s, j), [k, k, 0, k, c, np.float32(0)])
                r[1] = k
                r[2] += 1
                r[5] = np.float32(r[5] + c)
                if c > r[4]:
                    r[4], r[3] = c, k

    def update(self, logits, sources, windows, sites=None, conf=None):
        """One update: rows in any order of sources, each source's windows increasing.  conf: prior_ref.sigmoid_row of the logits, if
        the caller has it already.  Returns the sorted events."""
        x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, self.n_species)
        if conf is None:
            conf = prior_ref.sigmoid_row(x).reshape(x.shape)
        out = []
        for r in range(x.shape[0]):
            s, k = int(sources[r]), int(windows[r])
            assert 0 <= s < self.n_sources and self.last_window[s] < k < 2 ** 31, (s, k, self.last_window[s])
            self.last_window[s] = k
            prow = None if self.prior is None else self.prior[0][int(sites[r])]
            self._row(s, k, conf[r], prow, out)
        return sort_events(np.array(out, dtype=EVENT_DTYPE))

    def flush(self, source=-1):
        out = []
        for (s, j) in sorted(self.rec):
            if source < 0 or s == source:
                self._close(s, j, out)
        return sort_events(np.array(out, dtype=EVENT_DTYPE))

    def reset(self, source):
        for key in [key for key in self.rec if key[0] == source]:
            del self.rec[key]
        self.last_window[source] = -1

    def open_events(self, source=-1):
        return sum(1 for (s, _) in self.rec if source < 0 or s == source)
