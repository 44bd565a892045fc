"""The device's genotype summaries without a GPU: bt_diag_genotype_cluster runs the __host__ __device__ code of bt_gibbs_genotypes
(bayestyper_amd/csrc/bt_genotypes.hpp) on host arrays; every output must equal the host layer's getGenotypes (bth_cluster_genotypes), floats bit for
bit.  Hand-made clusters for every branch, then the oracle's collected samples of the batch tests/test_genotypes_cpu.py uses."""
import numpy as np
import pytest

import _oracle
from _genotypes_device import assert_cluster_equals_host, group_of_cluster, min_fraction, multiallelic_batch
from bayestyper_amd import lib
from bayestyper_amd.host import genotypes
from test_genotypes_cpu import _batch

NONE = 0xFFFF


def _cluster(S, hap_allele, num_alleles, has_dependency, entries, stats=None):
    """one cluster as (flat, res): hap_allele [H][V]; entries: list of (h1, h2, [count per sample]) — sorted here into bt_gibbs_result_fetch's order unless
    already given that way; stats: [S][A_total][3][4] (default: every allele with 20 k-mers observed completely)"""
    hap_allele = np.asarray(hap_allele, np.uint16).reshape(len(hap_allele), -1)
    H, V = hap_allele.shape
    A_total = int(np.sum(num_alleles))
    if stats is None:
        stats = np.zeros((S, A_total, 3, 4))
        stats[:, :, 0] = (5, 0, 20.0, 0)
        stats[:, :, 1] = (5, 0, 1.0, 0)
        stats[:, :, 2] = (5, 0, 12.5, 0)
    flat = {"S": S, "num_haplotypes": np.array([H], np.uint32), "num_variants": np.array([V], np.uint32), "hap_allele": hap_allele.reshape(-1),
            "var_num_alleles": np.asarray(num_alleles, np.uint16), "var_has_dependency": np.asarray(has_dependency, np.uint8)}
    res = {"dip_off": np.array([0, len(entries)], np.uint64), "h1": np.array([e[0] for e in entries], np.uint16), "h2": np.array([e[1] for e in entries], np.uint16),
           "freq": np.array([e[2] for e in entries], np.uint32).reshape(len(entries), S), "cell_off": np.array([0, S * A_total], np.uint64),
           "stats": np.asarray(stats, np.float64).reshape(S * A_total, 3, 4)}
    return flat, res


def _device(flat, res, ploidy, mf, min_gpp, min_kmers):
    S, H, V = flat["S"], int(flat["num_haplotypes"][0]), int(flat["num_variants"][0])
    w = lib.diag_genotype_cluster(S, H, V, flat["hap_allele"], flat["var_num_alleles"], flat["var_has_dependency"], res["h1"], res["h2"], res["freq"], res["stats"], ploidy, min_gpp,
                                  min_kmers, mf)
    assert (int(w[0]), int(w[1]), int(w[2])) == (1, V, S) and int(w[5]) == V
    voff = w[6:6 + V + 1].astype(np.int64)
    assert (np.diff(voff) > 0).all() and voff[-1] == len(w) and (voff % 2 == 0).all()
    parsed = lib.parse_genotype_words(w)
    assert len(parsed) == 1
    return parsed[0]


def _check(flat, res, ploidy, mf=None, min_gpp=0.99, min_kmers=1.0, what=""):
    S = flat["S"]
    mf = np.full(S, 0.5, np.float32) if mf is None else np.asarray(mf, np.float32)
    dev = _device(flat, res, ploidy, mf, min_gpp, min_kmers)
    return assert_cluster_equals_host(dev, flat, res, 0, np.asarray(ploidy, np.uint8), mf, min_gpp, min_kmers, what), dev


def test_ploidy_0_1_2_and_the_missing_allele():
    """a new test of the device route: fails without bt_diag_genotype_cluster"""
    # one variant with a dependency: alleles ref, alt, missing; haplotype 0 = ref, 1 = alt; 0xFFFF haplotypes map to the missing allele
    entries = [(0, 0, [90, 0, 7]), (0, 1, [10, 0, 7]), (0, NONE, [0, 95, 0]), (1, NONE, [0, 5, 0]), (NONE, NONE, [0, 0, 86])]
    flat, res = _cluster(3, [[0], [1]], [3], [1], entries)
    host, dev = _check(flat, res, [2, 1, 0], min_gpp=0.9)
    assert tuple(host["estimate"][0, 0]) == (0, 0) and tuple(host["estimate"][0, 1]) == (0, NONE) and tuple(host["estimate"][0, 2]) == (NONE, NONE)
    assert host["total_count"][0] == 3 and dev["gpp"][0, 2].sum() == 0
    # the same samples read as diploid everywhere: the null diplotype is the homozygous missing allele
    host, _ = _check(flat, res, [2, 2, 2], min_gpp=0.8)
    assert tuple(host["estimate"][0, 2]) == (2, 2)


@pytest.mark.parametrize("dep", [0, 1])
@pytest.mark.parametrize("A", [2, 3, 5])
def test_allele_counts_with_and_without_dependency(A, dep):
    rng = np.random.default_rng(100 * A + dep)
    S, V, H = 4, 3, 7
    na = [A, 2 + dep, A]
    real = [a - d for a, d in zip(na, [dep, dep, 0])]   # alleles a haplotype can carry (the missing allele of a dependent variant is never on a candidate)
    dependency = [dep, dep, 0]
    hap_allele = np.stack([rng.integers(0, real[v], H) for v in range(V)], axis=1)
    hap_allele[:, 2] = np.minimum(hap_allele[:, 2], A - 2)   # the last allele of the third variant stays uncovered
    pairs = [(a, b) for a in range(H) for b in range(a, H)] + [(a, NONE) for a in range(H)] + [(NONE, NONE)]
    pick = sorted(rng.choice(len(pairs), 12, replace=False))
    entries = [(pairs[i][0], pairs[i][1], list(rng.integers(0, 40, S) * rng.integers(0, 2, S))) for i in pick]
    stats = rng.random((S, sum(na), 3, 4)) * 3
    stats[:, :, :, 0] = rng.integers(0, 3, (S, sum(na), 3))   # counts of 0: getMean is -1
    flat, res = _cluster(S, hap_allele, na, dependency, entries, stats)
    for ploidy in ([2, 2, 2, 2], [1, 2, 0, 1]):
        host, _ = _check(flat, res, ploidy, mf=[0.5, 0.1, 0.9, 0.5], min_gpp=0.3, min_kmers=1.5, what=(A, dep, ploidy))
        assert host["non_covered"][2, A - 1] == 1 and host["non_covered"][0, A - 1] == (0 if dep else host["non_covered"][0, A - 1])


def test_tie_for_best_is_no_call():
    flat, res = _cluster(2, [[0], [1]], [2], [0], [(0, 0, [50, 60]), (0, 1, [50, 40])])
    host, dev = _check(flat, res, [2, 2], min_gpp=0.4)
    assert tuple(host["estimate"][0, 0]) == (NONE, NONE) and tuple(host["estimate"][0, 1]) == (0, 0)
    assert dev["best"][0, 0] == np.float32(0.5) and host["total_count"][0] == 2


def test_best_just_below_and_exactly_at_the_minimum_posterior():
    flat, res = _cluster(3, [[0], [1]], [2], [0], [(0, 0, [3, 74, 75]), (0, 1, [1, 26, 25])])
    host, _ = _check(flat, res, [2, 2, 2], min_gpp=0.75)                       # 0.75 exactly at the minimum: called; 0.74: not
    assert [tuple(e) for e in host["estimate"][0]] == [(0, 0), (NONE, NONE), (0, 0)]
    inside = np.float32(0.75) * (np.float32(1) + np.float32(50) * np.finfo(np.float32).eps)    # above 0.75, inside floatCompare's tolerance: still called
    host, _ = _check(flat, res, [2, 2, 2], min_gpp=float(inside))
    assert tuple(host["estimate"][0, 0]) == (0, 0)
    outside = np.float32(0.75) * (np.float32(1) + np.float32(200) * np.finfo(np.float32).eps)
    host, _ = _check(flat, res, [2, 2, 2], min_gpp=float(outside))
    assert tuple(host["estimate"][0, 0]) == (NONE, NONE)


def test_allele_filters_on_the_best_and_on_another_allele():
    S, A = 4, 3
    stats = np.zeros((S, A, 3, 4))
    stats[:, :, 0] = (5, 0, 20.0, 0)
    stats[:, :, 1] = (5, 0, 1.0, 0)
    stats[0, 0, 0, 2] = 0.5      # sample 0: too few k-mers (NAK) on the best genotype's allele
    stats[1, 2, 0, 2] = 0.5      # sample 1: NAK on an allele outside the best genotype
    stats[2, 1, 1, 2] = 0.1      # sample 2: too low a fraction (FAK) on the best genotype's second allele
    stats[3, 1, 0, 2] = 0.0      # sample 3: a count mean of 0 — NAK, and FAK is skipped although the fraction is low
    stats[3, 1, 1, 2] = 0.1
    entries = [(0, 0, [1, 1, 1, 1]), (0, 1, [97, 97, 97, 97]), (1, 2, [2, 2, 2, 2])]
    flat, res = _cluster(S, [[0], [1], [2]], [A], [0], entries, stats)
    host, _ = _check(flat, res, [2] * S, mf=[0.5] * S, min_gpp=0.9)
    assert host["filters"][0, 0].tolist() == [1, 0, 0] and host["filters"][0, 1].tolist() == [0, 0, 1]
    assert host["filters"][0, 2].tolist() == [0, 2, 0] and host["filters"][0, 3].tolist() == [0, 1, 0]
    assert [tuple(e) for e in host["estimate"][0]] == [(NONE, NONE), (0, 1), (NONE, NONE), (NONE, NONE)]
    assert host["total_count"][0] == 2 and host["alt_counts"][0].tolist() == [1, 0, 0]
    # an allele that was never sampled carries no filter, whatever its statistics
    entries = [(0, 0, [100, 100, 100, 100])]
    flat, res = _cluster(S, [[0], [1], [2]], [A], [0], entries, stats)
    host, _ = _check(flat, res, [2] * S, mf=[0.5] * S, min_gpp=0.9)
    assert host["filters"][0, 1].tolist() == [0, 0, 0] and host["filters"][0, 0].tolist() == [1, 0, 0]


def test_variant_without_a_call_has_total_count_zero():
    flat, res = _cluster(2, [[0, 0], [1, 1]], [2, 2], [0, 0], [(0, 0, [40, 10]), (0, 1, [35, 50]), (1, 1, [25, 40])])
    host, _ = _check(flat, res, [2, 1], min_gpp=0.99)
    assert (host["total_count"] == 0).all() and (host["alt_freq"] == 0).all() and (host["estimate"] == NONE).all()


def test_sums_inside_float_compare_tolerance_follow_the_entry_order():
    """two genotypes with sums 90 000 and 90 001 — different integers that floatCompare takes for equal — reached through several entries each: the
    running maximum depends on the order of the increments, and the device walks bt_gibbs_result_fetch's (h1, h2) order like the host"""
    # haplotypes 0..2 carry allele 0, 3..5 allele 1; (h1, h2) order interleaves hom-ref entries (h2 < 3) and het entries (h2 >= 3)
    hap_allele = [[0], [0], [0], [1], [1], [1]]
    keys = [(0, 0), (0, 1), (0, 3), (0, 4), (1, 1), (1, 3), (2, 2), (2, 5)]
    hom = [k for k in keys if k[1] < 3]
    tables = [{(0, 0): 30000, (0, 1): 30000, (1, 1): 20000, (2, 2): 10000, (0, 3): 45000, (0, 4): 45000, (1, 3): 1, (2, 5): 0},      # het first reaches 90 001
              {(0, 0): 89999, (0, 1): 0, (1, 1): 0, (2, 2): 1, (0, 3): 1, (0, 4): 1, (1, 3): 89998, (2, 5): 1},
              {(0, 0): 1, (0, 1): 1, (1, 1): 1, (2, 2): 89997, (0, 3): 90000, (0, 4): 0, (1, 3): 0, (2, 5): 1}]
    calls = []
    for t in tables:
        assert sum(t[k] for k in hom) == 90000 and sum(t[k] for k in keys if k not in hom) == 90001
        flat, res = _cluster(1, hap_allele, [2], [0], [(a, b, [t[(a, b)]]) for a, b in keys])
        host, dev = _check(flat, res, [2], min_gpp=0.4, what=t)
        assert host["gpp"][0, 0, 0] != host["gpp"][0, 0, 1]
        calls.append(tuple(int(x) for x in host["estimate"][0, 0]))
    assert (NONE, NONE) in calls   # at least one order ends with both genotypes in the set of best ones


def _diag_batch_against_host(oracle, flat, ploidy, mf, what):
    """the oracle's collected samples of `flat` (seed 11, 3 chains, burn-in 10, 40 iterations), every cluster through the diagnostic entry -> calls, non-covered alleles"""
    S = flat["S"]
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    og = _oracle.OrcGibbs(oracle, flat, lut_g, lut_n, seed=11, chains=3, burn=10, iters=40)
    og.run(4)
    res = og.results()
    og.close()
    group = group_of_cluster(flat)
    called = uncovered = 0
    for c in range(flat["num_clusters"]):
        H, V = int(flat["num_haplotypes"][c]), int(flat["num_variants"][c])
        hv0 = int(np.sum(flat["num_haplotypes"][:c].astype(np.int64) * flat["num_variants"][:c].astype(np.int64)))
        v0 = int(np.sum(flat["num_variants"][:c]))
        e0, e1 = int(res["dip_off"][c]), int(res["dip_off"][c + 1])
        w = lib.diag_genotype_cluster(S, H, V, flat["hap_allele"][hv0:hv0 + H * V], flat["var_num_alleles"][v0:v0 + V], flat["var_has_dependency"][v0:v0 + V], res["h1"][e0:e1],
                                      res["h2"][e0:e1], res["freq"][e0:e1], res["stats"][int(res["cell_off"][c]):int(res["cell_off"][c + 1])], ploidy[group[c]], 0.99, 1.0, mf)
        host = assert_cluster_equals_host(lib.parse_genotype_words(w)[0], flat, res, c, ploidy[group[c]], mf, what=what)
        called += int((host["estimate"][:, :, 0] != NONE).sum())
        uncovered += int(host["non_covered"].sum())
    return called, uncovered


def test_oracle_samples_of_the_mixed_batch(oracle):
    """the collected samples test_genotypes_cpu.py summarises (more than 10 called genotypes)"""
    flat, ploidy = _batch(3)
    called, _ = _diag_batch_against_host(oracle, flat, ploidy, genotypes.min_fraction_observed_kmers([15.0] * 3), "mixed batch")
    assert called > 10


def test_oracle_samples_of_a_multiallelic_batch(oracle):
    """synth's multi-allelic option: 2 to 6 alleles per variant with and without the missing allele, alleles no candidate covers"""
    flat, ploidy = multiallelic_batch(3, 3)
    assert set(range(2, 8)) <= set(int(a) for a in flat["var_num_alleles"])
    called, uncovered = _diag_batch_against_host(oracle, flat, ploidy, min_fraction(3), "multi-allelic batch")
    assert called > 10 and uncovered > 0


def test_multiallelic_option_of_make_cluster():
    """(calls without the option draw what they drew before: the frozen fixtures of tests/golden/ are generated through them)"""
    from bayestyper_amd import synth

    x = synth.make_cluster(np.random.default_rng(3), 3, 6, 2, flank_kmers=1, ic_kmers=1)
    assert (x.var_num_alleles == 2).all() and x.hap_allele.max() == 1
    z = synth.make_cluster(np.random.default_rng(3), 2, 9, 2, has_dependency=True, alleles=[3, 5])
    assert z.var_num_alleles.tolist() == [4, 6] and z.hap_allele[:, 0].max() == 2 and z.hap_allele[:, 1].max() == 4 and (z.hap_allele[0] == 0).all()
    assert len({tuple(h) for h in z.hap_allele}) == 9
    spec = synth.edge_group(np.random.default_rng(1), dict(V=2, H=4, alleles=[2, 6], dep=True))
    assert spec.clusters[0].var_num_alleles.tolist() == [3, 7]


def test_diag_entry_rejects_null_arguments_and_small_buffers():
    import ctypes as C

    n = C.c_uint64()
    assert lib.bt_diag_genotype_cluster(1, 1, 1, None, None, None, 0, None, None, None, None, None, None, None, 0, C.byref(n)) != 0
    assert "null argument" in lib.bt_last_error().decode()
    flat, res = _cluster(1, [[0], [1]], [2], [0], [(0, 1, [5])])
    f, keep = lib._genotype_filters(0.9, 1.0, [0.5])
    arrs = [np.ascontiguousarray(flat[k]) for k in ("hap_allele", "var_num_alleles", "var_has_dependency")] + [res["h1"], res["h2"], res["freq"].reshape(-1), res["stats"].reshape(-1),
                                                                                                                np.array([2], np.uint8)]
    p = [a.ctypes.data for a in arrs]
    small = np.zeros(4, np.uint32)
    assert lib.bt_diag_genotype_cluster(1, 2, 1, p[0], p[1], p[2], 1, p[3], p[4], p[5], p[6], p[7], C.addressof(f), small.ctypes.data, 4, C.byref(n)) != 0
    assert "buffer too small" in lib.bt_last_error().decode() and n.value > 4 and not small.any()
