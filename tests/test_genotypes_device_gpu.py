"""bt_gibbs_genotypes: the genotype summaries of a launch computed on the device against the host layer's getGenotypes over the same sampler's
results (bayestyper_amd.host.genotypes.cluster_genotypes over Gibbs.results()), every array of every cluster, floats bit for bit.
Every sampler runs 3 chains x (10 + 40) sweeps."""
import ctypes as C
import re

import numpy as np
import pytest

import _oracle
from _genotypes_device import assert_cluster_equals_host, group_of_cluster, min_fraction, mixed_batch, multiallelic_batch

pytestmark = pytest.mark.gpu

KW = dict(seed=11, chains=3, burn=10, iters=40)
MIN_GPP, MIN_KMERS = 0.99, 1.0


def check_string(w, flat):
    """header = (C, sum V, S); cluster table = the clusters' variants; record offsets even, strictly increasing, the last one = the string's length"""
    Cn, NV = int(flat["num_clusters"]), int(np.sum(flat["num_variants"]))
    assert (int(w[0]), int(w[1]), int(w[2]), int(w[3])) == (Cn, NV, flat["S"], 0)
    assert np.array_equal(w[4:4 + Cn + 1], np.concatenate([[0], np.cumsum(flat["num_variants"])]).astype(np.uint32))
    voff = w[5 + Cn:5 + Cn + NV + 1].astype(np.int64)
    assert (np.diff(voff) > 0).all() and int(voff[-1]) == len(w) and (voff % 2 == 0).all() and int(voff[0]) >= 5 + Cn + NV + 1


def check_against_host(g, flat, ploidy, mf, what=""):
    """-> (the string, the sampler's results): every cluster of the string equals the host's summaries of g.results()"""
    from bayestyper_amd import lib

    res = g.results()
    w = g.genotypes(MIN_GPP, MIN_KMERS, mf)
    check_string(w, flat)
    parsed = lib.parse_genotype_words(w)
    assert len(parsed) == flat["num_clusters"]
    group = group_of_cluster(flat)
    called = 0
    for c in range(flat["num_clusters"]):
        host = assert_cluster_equals_host(parsed[c], flat, res, c, ploidy[group[c]], mf, MIN_GPP, MIN_KMERS, what)
        called += int((host["estimate"][:, :, 0] != 0xFFFF).sum())
    return w, res, called


def same_results(a, b):
    return all(np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k], b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]) for k in a)


@pytest.mark.parametrize("S", [1, 3, 10])
def test_mixed_batch_equals_host(gpu_ctx, oracle, S):
    from bayestyper_amd import lib

    flat, ploidy = mixed_batch(S)
    g = lib.Gibbs(gpu_ctx, flat, *_oracle.build_luts(oracle, S), **KW)
    g.run()
    before = g.results()
    w, res, called = check_against_host(g, flat, ploidy, min_fraction(S), what=f"S={S}")
    assert called > (10 if S >= 3 else 3)
    # the call does not disturb the sampler, and a second call returns the same string
    assert same_results(before, res) and same_results(before, g.results())
    assert np.array_equal(w, g.genotypes(MIN_GPP, MIN_KMERS, min_fraction(S)))
    # other filters: another string over the same samples, still the host's
    mf = np.full(S, 0.999, np.float32)
    w2 = g.genotypes(0.5, 30.0, mf)
    parsed, group = lib.parse_genotype_words(w2), group_of_cluster(flat)
    for c in range(flat["num_clusters"]):
        assert_cluster_equals_host(parsed[c], flat, res, c, ploidy[group[c]], mf, 0.5, 30.0, "strict filters")
    g.close()


@pytest.mark.parametrize("n_small", [3, 70])
def test_multiallelic_edge_batch_equals_host(gpu_ctx, oracle, n_small):
    """A = 2 .. 6, V = 1 .. 5, H = 1 / 2 / 33 / 40, with and without dependency; 11 groups in narrow tiles, and 78 groups: a full tile of 64 two-haplotype groups, its
    partial successor and the narrow tiles — the (variant, sample) cells do not fill the last workgroup"""
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = multiallelic_batch(S, n_small)
    A = flat["var_num_alleles"]
    assert set(range(2, 8)) <= set(int(a) for a in A) and set(int(v) for v in flat["num_variants"]) >= {1, 2, 3, 4, 5} and {1, 2, 33, 40} <= set(int(h) for h in flat["num_haplotypes"])
    g = lib.Gibbs(gpu_ctx, flat, *_oracle.build_luts(oracle, S), **KW)
    g.run()
    _, _, called = check_against_host(g, flat, ploidy, min_fraction(S), what=f"n_small={n_small}")
    assert called > 5
    g.close()


def ordered_cells(err):
    m = re.search(r"bt_gibbs_genotypes: (\d+) clusters, (\d+) variants, (\d+) cells \((\d+) walked in \(h1, h2\) order, ordered from (\d+) collected sweeps\)", err)
    assert m, err
    return int(m.group(3)), int(m.group(4)), int(m.group(5))


@pytest.mark.parametrize("ordered_from", [None, 121, 120, 1])
def test_both_sides_of_the_entry_order_threshold(gpu_ctx, oracle, monkeypatch, capfd, ordered_from):
    """cells whose sample collected fewer sweeps than the threshold (83 887: below it the order of the entries cannot matter) visit the table as it lies, the
    others in bt_gibbs_result_fetch's order; BT_GENOTYPES_ORDERED_FROM lowers the threshold.  Every sample here collects 3 x 40 = 120 sweeps."""
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = multiallelic_batch(S, 3)
    g = lib.Gibbs(gpu_ctx, flat, *_oracle.build_luts(oracle, S), **KW)
    g.run()
    monkeypatch.setenv("BT_GIBBS_DEBUG", "1")
    if ordered_from is None:
        monkeypatch.delenv("BT_GENOTYPES_ORDERED_FROM", raising=False)
    else:
        monkeypatch.setenv("BT_GENOTYPES_ORDERED_FROM", str(ordered_from))
    capfd.readouterr()
    check_against_host(g, flat, ploidy, min_fraction(S), what=f"ordered_from={ordered_from}")
    cells, ordered, threshold = ordered_cells(capfd.readouterr().err)
    assert cells == int(np.sum(flat["num_variants"])) * S
    assert threshold == (83887 if ordered_from is None else ordered_from)
    assert ordered == (cells if ordered_from in (120, 1) else 0)
    g.close()


def test_after_a_noise_drivers_loop(gpu_ctx, oracle):
    """noise_iteration with collection, and a resident chain begun, stepped and ended: the summaries of what those collected"""
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = mixed_batch(S)
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    n_it, first_collect = 9, 3
    tables = [_oracle.build_luts(oracle, S, noise_rate=0.02 + 0.03 * i)[1] for i in range(n_it)]
    kw = dict(seed=77, chains=2, burn=first_collect, iters=n_it - first_collect, noise_seeding=1)
    ga, gb = lib.Gibbs(gpu_ctx, flat, lut_g, lut_n, **kw), lib.Gibbs(gpu_ctx, flat, lut_g, lut_n, **kw)
    resident = False
    for chain in range(2):
        ga.set_noise_lut(lut_n)
        ga.init_chain(chain)
        for it in range(n_it):
            ga.noise_iteration(tables[it] if it else None, it >= first_collect)
        gb.set_noise_lut(lut_n)
        gb.init_chain(chain)
        resident = gb.noise_chain_begin(n_it, first_collect)
        for it in range(n_it):
            if resident:
                gb.noise_chain_step(tables[it] if it else None)
            else:
                gb.noise_iteration(tables[it] if it else None, it >= first_collect)
        if resident:
            gb.noise_chain_end()
        if chain == 0:
            ga.reset_groups()
            gb.reset_groups()
    assert resident, "the batch should fit the GPU as one resident launch"
    wa, ra, _ = check_against_host(ga, flat, ploidy, min_fraction(S), "noise_iteration")
    wb, rb, _ = check_against_host(gb, flat, ploidy, min_fraction(S), "resident chain")
    assert same_results(ra, rb) and np.array_equal(wa, wb)
    ga.close()
    gb.close()


def test_fails_while_a_resident_chain_is_in_flight(gpu_ctx, oracle):
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = mixed_batch(S)
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    g = lib.Gibbs(gpu_ctx, flat, lut_g, lut_n, seed=5, chains=1, burn=1, iters=4, noise_seeding=1)
    g.set_noise_lut(lut_n)
    g.init_chain(0)
    assert g.noise_chain_begin(5, 1)
    for _ in range(2):   # (a chain may run its first iteration as ordinary launches: the resident launch is in flight from the second step on at the latest)
        g.noise_chain_step(None)
    with pytest.raises(lib.BtError, match=r"bt_gibbs_genotypes: a resident noise chain is in progress \(bt_gibbs_noise_chain_end\)"):
        g.genotypes(MIN_GPP, MIN_KMERS, min_fraction(S))
    for _ in range(3):   # the chain still ends normally
        assert g.noise_chain_step(None).sum() > 0
    g.noise_chain_end()
    check_against_host(g, flat, ploidy, min_fraction(S), "after the chain")
    g.close()


def test_sampler_over_a_permuted_selection_of_a_source(gpu_ctx, oracle):
    """records come in the SAMPLER's cluster order: the groups of a GibbsSource in a permuted selection"""
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = mixed_batch(S)
    src = lib.GibbsSource.from_batch(gpu_ctx, flat)
    G = flat["num_groups"]
    ids = np.random.default_rng(3).permutation(G)[: G // 2 + 3]
    g = src.sampler(KW, ids, *_oracle.build_luts(oracle, S))
    g.run()
    res = g.results()
    mf = min_fraction(S)
    w = g.genotypes(MIN_GPP, MIN_KMERS, mf)
    parsed = lib.parse_genotype_words(w)
    goff = np.asarray(flat["group_cluster_off"], np.int64)
    clusters = [(int(gi), c) for gi in ids for c in range(goff[gi], goff[gi + 1])]   # (group, cluster of the whole batch) in the sampler's order
    assert len(parsed) == len(clusters) == g.C and (int(w[0]), int(w[2])) == (g.C, S)
    assert int(w[1]) == sum(int(flat["num_variants"][c]) for _, c in clusters)
    for j, (gi, c) in enumerate(clusters):
        # the host's summaries of cluster j of the sampler's results, read with cluster c's description in the whole batch
        fake = {k: np.zeros(flat["num_clusters"] + 1, np.uint64) for k in ("dip_off", "cell_off")}
        for k in fake:
            fake[k][c], fake[k][c + 1] = res[k][j], res[k][j + 1]
        assert_cluster_equals_host(parsed[j], flat, dict(res, **fake), c, ploidy[gi], mf, MIN_GPP, MIN_KMERS, "permuted source")
    g.close()
    src.close()


def test_errors(gpu_ctx, oracle):
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = mixed_batch(S)
    g = lib.Gibbs(gpu_ctx, flat, *_oracle.build_luts(oracle, S), **KW)
    with pytest.raises(lib.BtError, match="bt_gibbs_genotypes: nothing was collected yet"):
        g.genotypes(MIN_GPP, MIN_KMERS, min_fraction(S))
    g.init_chain(0)
    g.sweep(5, False)   # sweeps without collection leave nothing to summarise either
    with pytest.raises(lib.BtError, match="bt_gibbs_genotypes: nothing was collected yet"):
        g.genotypes(MIN_GPP, MIN_KMERS, min_fraction(S))
    p, n = lib.vp(), C.c_uint64()
    f, keep = lib._genotype_filters(MIN_GPP, MIN_KMERS, min_fraction(S))
    for args in ((None, C.addressof(f), C.byref(p), C.byref(n)), (g.h, None, C.byref(p), C.byref(n)), (g.h, C.addressof(f), None, C.byref(n)), (g.h, C.addressof(f), C.byref(p), None)):
        assert lib.bt_gibbs_genotypes(*args) != 0 and "bt_gibbs_genotypes: null argument" in lib.bt_last_error().decode()
    f.min_fraction_observed_kmers = None
    assert lib.bt_gibbs_genotypes(g.h, C.addressof(f), C.byref(p), C.byref(n)) != 0 and "null argument" in lib.bt_last_error().decode()
    g.sweep(2, True)
    check_against_host(g, flat, ploidy, min_fraction(S), "two collected sweeps")
    g.close()
