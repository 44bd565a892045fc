"""Shared by the tests of the device genotype summaries (bt_gibbs_genotypes / bt_diag_genotype_cluster): the comparison of one cluster's parsed
records with the host layer's getGenotypes (bayestyper_amd.host.genotypes.cluster_genotypes), floats bit for bit."""
import numpy as np

from bayestyper_amd.host import genotypes

HOST_KEYS = ("gpp", "app", "filters", "estimate", "gq", "total_count", "alt_counts", "alt_freq", "acp", "max_alt_acp", "non_covered", "num_alleles")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def assert_cluster_equals_host(dev, flat, res, c, ploidy, min_fraction, min_gpp=0.99, min_kmers=1.0, what=""):
    """dev: parse_genotype_words(...)[i] for cluster c of (flat, res); every array of the host's dictionary must be equal, floats bitwise"""
    host = genotypes.cluster_genotypes(flat, res, c, ploidy, min_fraction, min_gpp, min_kmers)
    assert set(HOST_KEYS) <= set(host) and set(host) <= set(dev)
    for k in host:
        assert host[k].shape == dev[k].shape and host[k].dtype == dev[k].dtype, (what, c, k, host[k].shape, dev[k].shape)
        assert np.array_equal(_bits(host[k]), _bits(dev[k])), (what, c, k, host[k], dev[k])
    assert np.array_equal(dev["ploidy"], np.asarray(ploidy, np.uint8)), (what, c)
    # the best posterior is the largest genotype posterior (0 for ploidy 0); the k-mer means are KmerStats::getMean of the cell's three statistics
    V, S = host["gq"].shape
    A = host["num_alleles"].astype(np.int64)
    v0 = int(np.sum(flat["num_variants"][:c]))
    assert np.array_equal(dev["has_dependency"], np.asarray(flat["var_has_dependency"][v0:v0 + V], np.uint8)), (what, c)
    stats = np.asarray(res["stats"][int(res["cell_off"][c]):int(res["cell_off"][c + 1])], np.float64).reshape(S, int(A.sum()), 3, 4)
    base = np.concatenate([[0], np.cumsum(A)])
    for v in range(V):
        for s in range(S):
            want_best = host["gpp"][v, s].max() if host["gpp"][v, s].size and ploidy[s] else np.float32(0)
            # (the running maximum keeps the value it had when a genotype inside floatCompare's tolerance joined the set: equal up to that tolerance;
            #  the exact value is checked through gq, which the parser derives from it)
            assert abs(float(dev["best"][v, s]) - float(want_best)) <= 100 * float(np.finfo(np.float32).eps) * float(want_best), (what, c, v, s)
            cell = stats[s, base[v]:base[v] + A[v]]
            means = np.where(cell[:, :, 0] == 0, -1.0, cell[:, :, 2])
            assert np.array_equal(_bits(means), _bits(dev["kmer_means"][v, s, :A[v]])), (what, c, v, s)
    return host


def group_of_cluster(flat):
    goff = np.asarray(flat["group_cluster_off"], np.int64)
    return np.repeat(np.arange(len(goff) - 1), goff[1:] - goff[:-1])


def mixed_batch(S):
    """the composition of tests/test_genotypes_cpu.py's batch (10 shape-A, 4 shape-B, 2 nested shape-C groups) at any S, ploidy 0 / 1 / 2 mixed"""
    from bayestyper_amd import synth

    rng = np.random.default_rng(4)
    groups = ([synth.group_shape_A(rng, i) for i in range(10)] + [synth.group_shape_B(rng, 100 + i) for i in range(4)] +
              [synth.group_shape_C(rng, 200 + 3 * i, root_H=8, root_kpa=60) for i in range(2)])
    ploidy = np.full((len(groups), S), 2, np.uint8)
    ploidy[::4, min(1, S - 1)] = 1
    ploidy[3, min(2, S - 1)] = 0
    return synth.flatten(groups, S, rng, ploidy=ploidy, gender=([0, 1, 1] * 4)[:S]), ploidy


def multiallelic_batch(S, n_small, seed=9):
    """clusters with 2 to 6 alleles per variant, 1 to 5 variants, 1 / 2 / 33 / 40 haplotype candidates, with and without the missing allele of
    has_dependency, a nested group — and n_small two-haplotype groups in front, so that the tiles are narrower or wider than 64 groups"""
    from bayestyper_amd import synth

    specs = [dict(V=1, H=2, alleles=2, dep=bool(i % 3 == 1), kpa=12) for i in range(n_small)]
    specs += [dict(V=1, H=1, alleles=2, kpa=12), dict(V=1, H=1, alleles=3, dep=True, kpa=12), dict(V=2, H=2, alleles=3, dep=True, kpa=12), dict(V=3, H=33, alleles=[2, 4, 6], kpa=12),
              dict(V=5, H=40, alleles=[2, 3, 4, 5, 6], dep=True, kpa=12), dict(V=4, H=33, alleles=5, dep=True, kpa=12), dict(V=2, H=40, alleles=6, kpa=12),
              dict(V=3, H=8, alleles=3, kpa=12, kids=[dict(V=2, H=4, alleles=3, kpa=12), dict(V=1, H=2, alleles=2, kpa=12)])]
    rng = np.random.default_rng(seed)
    ploidy = rng.choice(np.array([0, 1, 2, 2, 2], np.uint8), size=(len(specs), S))
    return synth.make_edge_batch(specs, S, seed, ploidy=ploidy, gender=([0, 1, 1] * 4)[:S]), ploidy


def min_fraction(S):
    from bayestyper_amd.host import genotypes

    return genotypes.min_fraction_observed_kmers([15.0, 9.0, 30.0, 2.0][:S] + [15.0] * max(0, S - 4))
