"""Helpers of the batched best-path search tests (bt_find_paths_samples): a batch of clusters with one Bloom filter per sample, as an oracle twin and a
device twin, the oracle's rows after the samples in any order, and the device search as any sequence of sample() / samples() calls."""
import numpy as np

import _oracle  # noqa: F401
from _oracle import OrcBloom
from test_find_paths_wave_gpu import K, _clusters, _sample_kmers, _seeds

__all__ = ["K", "Case", "clusters", "seeds"]

clusters, seeds = _clusters, _seeds


class Case:
    """num_samples filters over one batch of clusters.  The seed row of a sample belongs to the sample, not to its place in a call: sample s always searches
    with seeds(C, s), whatever the order."""

    def __init__(self, gpu_ctx, oracle, rng, gs, truth, flat, max_haps, fpr, haps, num_samples=3):
        from bayestyper_amd import lib

        self.oracle, self.gs, self.flat, self.max_haps, self.num_samples = oracle, gs, flat, max_haps, num_samples
        self.orc_blooms, self.blooms = [], []
        for _ in range(num_samples):
            mem = _sample_kmers(oracle, rng, gs, truth, haps)
            ob = OrcBloom(oracle, len(mem), fpr, K)
            gb = lib.Bloom.create(gpu_ctx, len(mem), fpr, K, threaded=False)
            ob.insert(oracle.unpack(mem, K))
            gb.insert(mem)
            self.orc_blooms.append(ob)
            self.blooms.append(gb)
        self._expect = {}

    def seed_rows(self, order):
        return np.stack([_seeds(len(self.gs), s) for s in order])

    def expect(self, order=None):
        """the oracle's rows per cluster after findSamplePaths + addPathIndices of the samples in `order` (default 0 .. S-1), computed once per order"""
        from _oracle import OrcGraphs

        order = tuple(range(self.num_samples) if order is None else order)
        if order not in self._expect:
            og = OrcGraphs(self.oracle, self.flat, K)
            rows = None
            for s in order:
                rows = og.find_sample_paths(self.orc_blooms[s], _seeds(len(self.gs), s), self.max_haps)
            self._expect[order] = [b.copy() for b in rows]
            og.close()
        return self._expect[order]

    def run(self, gpu_ctx, monkeypatch, wave_min, calls, num_samples=None):
        """the device search with BT_FIND_PATHS_WAVE_MIN = wave_min.  calls: an int s is sample(s), a list of ints is one samples() call over them
        -> (rows per cluster at the end, info(), batch_info(), batch_bytes(2) before the first call)"""
        from bayestyper_amd import lib

        monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", str(wave_min))
        gf = lib.FindPaths(gpu_ctx, self.flat, K, self.max_haps, self.num_samples if num_samples is None else num_samples)
        try:
            for call in calls:
                if isinstance(call, int):
                    gf.sample(self.blooms[call], _seeds(len(self.gs), call))
                else:
                    gf.samples([self.blooms[s] for s in call], self.seed_rows(call))
            return gf.best_paths(), gf.info(), gf.batch_info()
        finally:
            gf.close()

    def assert_equal(self, got, expect):
        assert len(got) == len(expect) == len(self.gs)
        for c in range(len(self.gs)):
            assert expect[c].shape == got[c].shape and np.array_equal(expect[c], got[c]), c

    def differ(self, a, b):
        return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))

    def close(self):
        for b in self.blooms + self.orc_blooms:
            b.close()
