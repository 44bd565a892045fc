"""The best-path search with wide clusters on a wavefront each (find_paths_wave_kernel, BT_FIND_PATHS_WAVE_MIN): the routes bt_find_paths_info reports,
and the rows of the wave route against the oracle's findSamplePaths + addPathIndices and against the lane route."""
import numpy as np
import pytest

import _oracle  # noqa: F401
from _oracle import OrcBloom

pytestmark = pytest.mark.gpu

K = 31
NT = np.frombuffer(b"ACGT", np.uint8)


def _clusters(rng, sizes, max_paths=3, nested=True, kinds=None):
    from bayestyper_amd import synth_graphs

    kw = {} if kinds is None else {"kinds": kinds}
    gs = [synth_graphs.random_cluster(rng, K, int(n), max_paths, nested_cluster=(700 + i) if nested and i % 3 == 1 else None, **kw) for i, n in enumerate(sizes)]
    truth = [g.paths.copy() for g in gs]
    for g in gs:
        g.paths = None
    return gs, truth, synth_graphs.flatten(gs)


def _sample_kmers(oracle, rng, gs, truth, haps):
    """the sample's reads: `haps` haplotypes per cluster (random best-path rows), 10 % of their k-mers unobserved"""
    rows = [truth[i][rng.integers(len(truth[i]), size=haps)] for i in range(len(gs))]
    text = np.concatenate([np.concatenate([NT[g.seq[v]] for v in range(len(g.seq)) if rows[i][h, v]] + [np.frombuffer(b"N", np.uint8)])
                           for i, g in enumerate(gs) for h in range(haps)])
    km, va = oracle.kmers_from_sequence(text.tobytes(), K)
    mem = np.unique(km[va == 1], axis=0)
    return mem[rng.random(len(mem)) > 0.1]


def _seeds(n, s):
    return (4242 + (np.arange(n) + 1) * (s + 1) + np.arange(n)).astype(np.uint32)   # prng_seed + (group+1)*(sample+1) + cluster


class _Case:
    """two samples' filters (oracle + device twins) and the oracle's rows after each sample, computed once per batch"""

    def __init__(self, gpu_ctx, oracle, rng, gs, truth, flat, max_haps, fpr, haps, num_samples=2):
        from _oracle import OrcGraphs
        from bayestyper_amd import lib

        self.gs, self.flat, self.max_haps, self.num_samples = gs, flat, max_haps, num_samples
        self.blooms, self.expect = [], []
        og = OrcGraphs(oracle, flat, K)
        for s in range(num_samples):
            mem = _sample_kmers(oracle, rng, gs, truth, haps)
            ob = OrcBloom(oracle, len(mem), fpr, K)
            gb = lib.Bloom.create(gpu_ctx, len(mem), fpr, K, threaded=False)
            ob.insert(oracle.unpack(mem, K))
            gb.insert(mem)
            self.expect.append([b.copy() for b in og.find_sample_paths(ob, _seeds(len(gs), s), max_haps)])
            ob.close()
            self.blooms.append(gb)
        og.close()

    def run(self, gpu_ctx, monkeypatch, wave_min):
        """the device search with BT_FIND_PATHS_WAVE_MIN = wave_min: rows after each sample, and info() at the end"""
        from bayestyper_amd import lib

        monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", str(wave_min))
        gf = lib.FindPaths(gpu_ctx, self.flat, K, self.max_haps, self.num_samples)
        got = []
        for s in range(self.num_samples):
            gf.sample(self.blooms[s], _seeds(len(self.gs), s))
            got.append(gf.best_paths())
        st = gf.info()
        gf.close()
        return got, st

    def assert_equal(self, got, expect=None):
        expect = self.expect if expect is None else expect
        for s in range(self.num_samples):
            for c in range(len(self.gs)):
                assert expect[s][c].shape == got[s][c].shape and np.array_equal(expect[s][c], got[s][c]), (s, c)

    def close(self):
        for b in self.blooms:
            b.close()


def test_routes_reported(gpu_ctx, monkeypatch):
    """40 clusters of 1-7 variants and two of 40 variants (about 139 vertices): the planner's routes as bt_find_paths_info tells them"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(91)
    gs, _, flat = _clusters(rng, [int(rng.integers(1, 8)) for _ in range(40)] + [40, 40])
    nv = flat["vertex_off"][1:] - flat["vertex_off"][:-1]
    assert np.sort(nv)[-3] < 100 <= np.sort(nv)[-2]
    for wave_min, expect in ((100, 2), (0, 0), (1, len(gs))):
        monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", str(wave_min))
        gf = lib.FindPaths(gpu_ctx, flat, K, 32, 2)
        st = gf.info()
        gf.close()
        assert st.num_clusters == len(gs) and st.wave_min_vertices == wave_min
        assert st.num_wave_clusters == expect
        assert st.max_vertices == int(nv.max())
        assert st.max_candidate_paths == 0   # nothing searched yet


@pytest.mark.parametrize("max_haps,fpr,haps", [(32, 1e-6, 2), (3, 0.05, 6), (2, 0.3, 6)])
def test_wave_route_equals_oracle(gpu_ctx, oracle, monkeypatch, max_haps, fpr, haps):
    """every cluster on the wave kernel (one-vertex-list, nested of both parities, multi-allelic, one of 150 variants), two samples into the same rows"""
    rng = np.random.default_rng(52)
    gs, truth, flat = _clusters(rng, [int(rng.integers(1, 8)) for _ in range(40)] + [150], max_paths=max(3, haps))
    case = _Case(gpu_ctx, oracle, rng, gs, truth, flat, max_haps, fpr, haps)
    got, st = case.run(gpu_ctx, monkeypatch, 1)
    case.close()
    assert st.num_wave_clusters == st.num_clusters == len(gs) and st.max_vertices > 400
    assert st.max_candidate_paths >= 1
    case.assert_equal(got)
    assert sum(b.shape[0] for b in got[-1]) > len(gs)


def test_wave_route_equals_lane_route(gpu_ctx, oracle, monkeypatch):
    """the same batch (largest cluster 40 variants) on lanes only and on wavefronts only: equal cluster by cluster, and both equal to the oracle"""
    rng = np.random.default_rng(53)
    gs, truth, flat = _clusters(rng, [int(rng.integers(1, 8)) for _ in range(40)] + [40], max_paths=6)
    case = _Case(gpu_ctx, oracle, rng, gs, truth, flat, 3, 0.05, 6)
    lane, st_lane = case.run(gpu_ctx, monkeypatch, 0)
    wave, st_wave = case.run(gpu_ctx, monkeypatch, 1)
    mixed, st_mixed = case.run(gpu_ctx, monkeypatch, 100)   # both launches in one call
    case.close()
    assert st_lane.num_wave_clusters == 0 and st_lane.max_candidate_paths == 0
    assert st_wave.num_wave_clusters == len(gs) and st_mixed.num_wave_clusters == 1
    case.assert_equal(wave, lane)
    case.assert_equal(mixed, lane)
    case.assert_equal(lane)
    case.assert_equal(wave)


def test_wide_clusters_inside_the_batch(gpu_ctx, oracle, monkeypatch):
    """two clusters of 40 variants (about 139 vertices), each followed by ten small ones, threshold 100: a wide cluster's scratch region, score arrays
    included, lies between other clusters' regions — every region is placed by the one layout the kernels carve it with"""
    rng = np.random.default_rng(59)
    small = [int(rng.integers(1, 8)) for _ in range(20)]
    gs, truth, flat = _clusters(rng, [40] + small[:10] + [40] + small[10:], max_paths=6)
    nv = flat["vertex_off"][1:] - flat["vertex_off"][:-1]
    assert np.sort(nv)[-3] < 100 <= np.sort(nv)[-2]
    case = _Case(gpu_ctx, oracle, rng, gs, truth, flat, 3, 0.05, 6)
    mixed, st_mixed = case.run(gpu_ctx, monkeypatch, 100)
    lane, st_lane = case.run(gpu_ctx, monkeypatch, 0)
    case.close()
    assert st_mixed.num_wave_clusters == 2 and st_lane.num_wave_clusters == 0
    case.assert_equal(mixed)
    case.assert_equal(mixed, lane)


def test_more_than_64_candidate_paths_at_a_vertex(gpu_ctx, oracle, monkeypatch):
    """in-degree 3-4 with 32 kept paths per predecessor: the candidate paths of a vertex exceed a wavefront, so the strided lane loops and the
    first-match ballot take more than one pass"""
    rng = np.random.default_rng(57)
    gs, truth, flat = _clusters(rng, [12, 16, 20, 9], max_paths=6, nested=False, kinds=("multi", "multi", "multi", "snv"))
    case = _Case(gpu_ctx, oracle, rng, gs, truth, flat, 32, 0.05, 6, num_samples=1)
    got, st = case.run(gpu_ctx, monkeypatch, 1)
    case.close()
    print("max_candidate_paths", st.max_candidate_paths)
    assert st.max_candidate_paths > 64
    case.assert_equal(got)
