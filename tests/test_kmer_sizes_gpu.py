"""GPU tests of every k-dependent stage at k-mer sizes other than 55: path text, path Bloom insert, classification and candidates
(bt_paths_*), the multigroup pass on both order routes, the best-path search on its three entry routes (bt_find_paths_*), and the table's
text kernels (inter-cluster and parameter k-mers).  k = 15 and 31 keep a k-mer in one word, 32 fills it, 33 puts one symbol into the
second word and 64 fills both (no mask, no shift in the reverse complement).  Every comparison is exact, against the oracle; the multigroup
order is the real std::unordered_set<std::bitset<2k>>'s (oracle/oracle_kmer.cpp: make_kmer_set).  The inputs are small on purpose."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _oracle  # noqa: E402
import mg_wide_groups as MG  # noqa: E402
import test_kmer_sizes_cpu as KC  # noqa: E402
from _oracle import OrcBloom, OrcGraphs, OrcTable  # noqa: E402

pytestmark = pytest.mark.gpu
KS_GPU = [15, 31, 32, 33, 64]
NT = np.frombuffer(b"ACGT", np.uint8)


def _sorted_export(kmers, counts, meta):
    order = np.lexsort((kmers[:, 0], kmers[:, 1]))
    return kmers[order], counts[order], meta[order]


def _assert_tables_equal(gt, ot, what):
    gk, gc, gm = _sorted_export(*gt.export())
    wk, wc, wm = _sorted_export(*ot.export())
    assert np.array_equal(gk, wk), (what, len(gk), len(wk))
    assert np.array_equal(gm, wm) and np.array_equal(gc, wc), what
    return wk, wm


# ---------------------------------------------------------------------------------------------------------------------------------------
# path stages
# ---------------------------------------------------------------------------------------------------------------------------------------
def path_graphs(k):
    """14 clusters of 1..6 variants with at most 6 paths: two hold a nested cluster (one under a deletion's reference allele, one between
    variants), cluster 1 is a copy of cluster 0 (k-mers of two clusters); every variant kind occurs"""
    from bayestyper_amd import synth_graphs

    rng = np.random.default_rng(3100 + k)
    num_variants = [1, 2, 4, 3, 5, 6, 3, 5, 1, 2, 4, 6, 2, 3]
    nested = {2: 500, 7: 501}
    gs = [synth_graphs.random_cluster(rng, k, v, int(rng.integers(2, 7)), nested_cluster=nested.get(i)) for i, v in enumerate(num_variants)]
    gs[1] = copy.deepcopy(gs[0])
    gs[1].paths = synth_graphs.random_paths(gs[1], rng, 3)
    alts = [a for g in gs for v in g.variants for a in [v["alts"]]]
    assert any(len(a) == 3 for a in alts) and any(len(a) == 1 and a[0][0] == 1 and len(a[0][1]) == 1 for a in alts)        # multi-allelic, SNV
    assert any(len(a) == 1 and len(a[0][1]) > 1 for a in alts) and any(len(a) == 1 and 1 < a[0][0] < 40 for a in alts)    # insertion, deletion
    assert len(gs) == 14 and max(g.paths.shape[0] for g in gs) <= 6
    return gs, synth_graphs.flatten(gs)


@pytest.mark.parametrize("k", KS_GPU)
def test_path_stages(gpu_ctx, oracle, k):
    """countPathKmers / classifyPathKmers / getHaplotypeCandidates at size k: the number of windows and the path Bloom bit image, the
    classification counts, excluded flags and the table, and every field of the candidates bundle equal the oracle's"""
    from bayestyper_amd import lib

    S = 2
    gs, f = path_graphs(k)
    og = OrcGraphs(oracle, f, k)
    gp = lib.Paths(gpu_ctx, f, k)
    ob = OrcBloom(oracle, 50_000, 1e-3, k, threaded=False)
    gb = lib.Bloom.create(gpu_ctx, 50_000, 1e-3, k, threaded=False)
    assert og.count_kmers(ob) == gp.num_windows > 0
    gp.count_kmers(gb)
    gpu_ctx.sync()
    assert np.array_equal(gb.bits(0), ob.bits(0))
    # a count table holding part of the path k-mers, some with intercluster multiplicity, one decoy region
    ot, gt = OrcTable(oracle, S, k), lib.Table(gpu_ctx, 50_000, S, k)
    rng = np.random.default_rng(5)
    text = np.concatenate([np.concatenate([NT[g.seq[v]] for v in range(len(g.seq))] + [np.frombuffer(b"N", np.uint8)]) for g in gs[:6]])
    tb_o = OrcBloom(oracle, 50_000, 1e-3, k, threaded=True)
    tb_g = lib.Bloom.create(gpu_ctx, 50_000, 1e-3, k, threaded=True)
    km, va = oracle.kmers_from_sequence(text.tobytes(), k)
    members = np.unique(km[va == 1], axis=0)
    tb_o.insert(oracle.unpack(members, k))
    tb_g.insert(members)
    ot.count_intercluster(tb_o, text[: len(text) // 3].tobytes(), 0, 2, 1)
    gt.count_intercluster(tb_g, text[: len(text) // 3].tobytes(), 0, 2, 1)
    dec = text[len(text) // 3: len(text) // 3 + 200].tobytes()
    ot.count_intercluster(tb_o, dec, 1, 0, 0)
    gt.count_intercluster(tb_g, dec, 1, 0, 0)
    mg_members = members[rng.choice(len(members), 30, replace=False)]
    omg = OrcBloom(oracle, 30, 1e-4, k)
    gmg = lib.Bloom.create(gpu_ctx, 30, 1e-4, k, threaded=False)
    omg.insert(oracle.unpack(mg_members, k))
    gmg.insert(mg_members)
    n_o, ex_o = og.classify(ot, omg)
    n_g, ex_g = gp.classify(gt, gmg)
    assert np.array_equal(n_o, n_g) and np.array_equal(ex_o, ex_g) and ex_o.any() and not ex_o.all()
    wk, wm = _assert_tables_equal(gt, ot, "table after classify")
    assert (wm[:, 0] & 0x02).any() and (wm[:, 0] & 0x08).any() and (wm[:, 0] & 0x04).any()   # multicluster, decoy, multigroup
    ro = og.candidates(ot)
    rg = gp.candidates(gt)
    for name in ro:
        assert np.array_equal(ro[name], rg[name]), name
    assert len(ro["multi_idx"]) > 0 and len(ro["hapnest_idx"]) > 0 and len(ro["nestdep_var"]) > 0
    for x in (gp, og, gb, ob, gt, ot, tb_o, tb_g, omg, gmg):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# multigroup
# ---------------------------------------------------------------------------------------------------------------------------------------
CLUSTER_GROUP = np.array([0, 1, 2, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, 11, 11, 12, 13], np.uint32)


def multigroup_units(k):
    """the two units of test_kmer_gpu.py::test_path_multigroup_kmers at size k: groups of very different sizes, a cluster shared by two clusters
    of one group (not multigroup), by two groups (multigroup) and by the two units (in the filter already)"""
    from bayestyper_amd import synth_graphs

    rng = np.random.default_rng(4100 + k)
    units, shared = [], None
    for unit in range(2):
        sizes = [int(rng.integers(1, 5)) for _ in range(12)] + [40, 1, 2, 90, 3]      # variants per cluster: small groups after large ones
        gs = [synth_graphs.random_cluster(rng, k, v, int(rng.integers(2, 7))) for v in sizes]
        gs[3] = copy.deepcopy(gs[2])
        gs[3].paths = synth_graphs.random_paths(gs[3], rng, 3)
        gs[9] = copy.deepcopy(gs[5])
        gs[9].paths = synth_graphs.random_paths(gs[9], rng, 2)
        if unit == 0:
            shared = copy.deepcopy(gs[7])
        else:
            gs[1] = shared
        units.append(synth_graphs.flatten(gs))
    return units


@pytest.mark.parametrize("n_filter,fpr,threaded", [(1_000_000, 1e-7, True), (3000, 0.02, False)], ids=["roomy-filter", "undersized-filter"])
@pytest.mark.parametrize("k", KS_GPU)
def test_multigroup_both_routes(gpu_ctx, oracle, monkeypatch, k, n_filter, fpr, threaded):
    """countPathMultigroupKmers at size k over two units that share filter and table, with every group on a lane (BT_MG_WIDE_MIN unset) and
    every group on a workgroup (BT_MG_WIDE_MIN=1): table, num_path_kmers and filter bits equal the oracle's — which walks the real
    unordered_set<bitset<2k>> — after each unit, hence each other; bt_paths_multigroup_info reports the route of every group.  With the
    undersized filter most table entries are false positives of the moment, so a wrong order at this k changes the table."""
    from bayestyper_amd import lib

    units = multigroup_units(k)
    subs = list(range(0, 65536, 4099)) if threaded else [0]
    ob, ot = OrcBloom(oracle, n_filter, fpr, k, threaded=threaded), OrcTable(oracle, 1, k)
    want = []
    for f in units:
        og = OrcGraphs(oracle, f, k)
        n = og.count_multigroup(CLUSTER_GROUP, ob, ot)
        og.close()
        want.append((n, _sorted_export(*ot.export())[0], [ob.bits(s) for s in subs]))
    total = sum(w[0] for w in want)
    assert all(w[0] > 0 for w in want) and len(want[-1][1]) > 50
    if fpr > 1e-3:
        assert len(want[-1][1]) > 0.02 * total
    ob.close(), ot.close()
    for wide in (None, "1"):
        if wide is None:
            monkeypatch.delenv("BT_MG_WIDE_MIN", raising=False)
        else:
            monkeypatch.setenv("BT_MG_WIDE_MIN", wide)
        gb = lib.Bloom.create(gpu_ctx, n_filter, fpr, k, threaded=threaded)
        gt = lib.Table(gpu_ctx, 16 if fpr > 1e-3 else 200_000, 1, k)
        for u, f in enumerate(units):
            gp = lib.Paths(gpu_ctx, f, k)
            assert gp.count_multigroup(CLUSTER_GROUP, gb, gt) == want[u][0], (wide, u)
            info = gp.multigroup_info()
            gp.close()
            gk = _sorted_export(*gt.export())[0]
            assert np.array_equal(gk, want[u][1]), (wide, u, len(gk), len(want[u][1]))
            for s, bits in zip(subs, want[u][2]):
                assert np.array_equal(gb.bits(s), bits), (wide, u, s)
            assert info["num_groups"] == 14 and info["wide_min_kmers"] == (0 if wide is None else 1)
            assert info["num_wide_groups"] == (0 if wide is None else 14)          # every group holds k-mers
            assert (info["wide_scratch_bytes"] > 0) == (wide is not None) and info["max_group_kmers"] > 100
        gb.close(), gt.close()


@pytest.mark.parametrize("k", _oracle.KMER_SET_SIZES)
def test_kmer_set_orders_on_device(gpu_ctx, oracle, k):
    """bt_kmer_set_orders at every size the oracle holds the real container at, over the CPU test's group sequence up to 700 k-mers, with
    every group on a lane (wide_min 0) and on a workgroup (1): ranks and bucket counts equal the real container's"""
    from bayestyper_amd import lib

    sizes = KC.group_sizes(k)
    sizes = sizes[:sizes.index(700) + 1] if 700 in sizes else sizes
    groups, packed = KC.kmer_groups(oracle, k, sizes)
    want_order, want_buckets = oracle.kmer_set_orders(k, groups)
    for wide_min in (0, 1):
        ranks, final, stats = lib.kmer_set_orders(gpu_ctx, packed, k, 1, wide_min)
        for g, rank in enumerate(ranks):
            assert np.array_equal(MG.order_of(rank), want_order[g]), f"k = {k}, wide_min {wide_min}, group {g} ({sizes[g]} k-mers)"
        assert np.array_equal(final, want_buckets), (k, wide_min)
        assert stats["num_groups"] == len(sizes) and stats["num_wide_groups"] == (sum(1 for n in sizes if n) if wide_min else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# best-path search
# ---------------------------------------------------------------------------------------------------------------------------------------
def _seeds(n, s):
    return (4242 + (np.arange(n) + 1) * (s + 1) + np.arange(n)).astype(np.uint32)   # prng_seed + (group+1)*(sample+1) + cluster


def find_paths_case(oracle, k, max_haps, fpr):
    """20 clusters of 1..7 variants, two samples of two haplotypes each with 10 % of their k-mers unobserved: the flat graphs, the samples'
    k-mers and the oracle's rows after both samples"""
    from bayestyper_amd import synth_graphs

    rng = np.random.default_rng(5200 + k)
    gs = [synth_graphs.random_cluster(rng, k, int(rng.integers(1, 8)), 3, nested_cluster=(700 + i) if i % 3 == 1 else None) for i in range(20)]
    truth = [g.paths.copy() for g in gs]
    for g in gs:
        g.paths = None
    f = synth_graphs.flatten(gs)
    og = OrcGraphs(oracle, f, k)
    members, rows = [], None
    for s in range(2):
        pick = [truth[i][rng.integers(len(truth[i]), size=2)] for i in range(len(gs))]
        text = np.concatenate([np.concatenate([NT[g.seq[v]] for v in range(len(g.seq)) if pick[i][h, v]] + [np.frombuffer(b"N", np.uint8)])
                               for i, g in enumerate(gs) for h in range(2)])
        km, va = oracle.kmers_from_sequence(text.tobytes(), k)
        mem = np.unique(km[va == 1], axis=0)
        mem = mem[rng.random(len(mem)) > 0.1]
        ob = OrcBloom(oracle, len(mem), fpr, k)
        ob.insert(oracle.unpack(mem, k))
        rows = [r.copy() for r in og.find_sample_paths(ob, _seeds(len(gs), s), max_haps)]
        ob.close()
        members.append(mem)
    og.close()
    return f, members, rows


@pytest.mark.parametrize("max_haps,fpr", [(32, 1e-6), (2, 0.3)])
@pytest.mark.parametrize("k", KS_GPU)
def test_best_path_search_three_routes(gpu_ctx, oracle, monkeypatch, k, max_haps, fpr):
    """findSamplePaths + addPathIndices at size k for two samples, taken from bt_find_paths_sample on lanes, with
    BT_FIND_PATHS_WAVE_MIN=1 (every cluster on a wavefront) and from one bt_find_paths_samples call: the rows equal the oracle's, hence each
    other.  The sliding window of the search carries over from a vertex shorter than k and is refilled inside one longer than k; at k = 32,
    33 and 64 (either side of the one-word / two-word split of the window) the batch is checked to hold both."""
    from bayestyper_amd import lib

    f, members, want = find_paths_case(oracle, k, max_haps, fpr)
    C_ = f["num_clusters"]
    vlen = (f["seq_off"][1:] - f["seq_off"][:-1]).astype(np.int64)
    if k in (32, 33, 64):
        assert ((vlen > 0) & (vlen < k)).any() and (vlen > k).any()
    assert sum(r.shape[0] for r in want) > C_
    blooms = []
    for mem in members:
        gb = lib.Bloom.create(gpu_ctx, len(mem), fpr, k, threaded=False)
        gb.insert(mem)
        blooms.append(gb)
    seeds = np.stack([_seeds(C_, s) for s in range(2)])
    got = {}
    for route, wave_min in (("lanes", "0"), ("wavefronts", "1"), ("one call", "0")):
        monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", wave_min)
        gf = lib.FindPaths(gpu_ctx, f, k, max_haps, 2)
        if route == "one call":
            gf.samples(blooms, seeds)
        else:
            for s in range(2):
                gf.sample(blooms[s], seeds[s])
        got[route] = gf.best_paths()
        assert gf.info().num_wave_clusters == (C_ if route == "wavefronts" else 0)
        gf.close()
    for route, rows in got.items():
        for c in range(C_):
            assert rows[c].shape == want[c].shape and np.array_equal(rows[c], want[c]), (route, c)
    for gb in blooms:
        gb.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# table text kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def _genome(k):
    """20 000 nt with an N run and two repeats; regions (start, length, decoy): unsorted, one shorter than k, one decoy that overlaps the repeat"""
    rng = np.random.default_rng(6300 + k)
    genome = NT[rng.integers(0, 4, 20_000)].copy()
    genome[7_000:7_030] = ord("N")
    genome[15_000:15_400] = genome[1_000:1_400]          # a stretch of the second region again in the decoy
    genome[11_000:11_200] = genome[600:800]              # and a stretch of path k-mers twice in ordinary regions
    regions = [(6_000, 2_500, 0), (0, 3_000, 0), (14_900, 700, 1), (3_050, k - 1, 0), (10_000, 3_000, 0)]
    return genome, regions


@pytest.mark.parametrize("k", KS_GPU)
def test_table_text_kernels(gpu_ctx, oracle, k):
    """countInterclusterKmers and countInterclusterParameterKmers (fractions 0.05 and 1.0) at size k over regions of a small genome: the
    exported table — keys, multiplicities, flags — equals the oracle's"""
    from bayestyper_amd import lib

    genome, regions = _genome(k)
    path_k, path_v = oracle.kmers_from_sequence(genome[500:1_200].tobytes(), k)
    path = np.unique(path_k[path_v == 1], axis=0)
    ob = OrcBloom(oracle, len(path), 1e-3, k, threaded=True)
    ob.insert(oracle.unpack(path, k))
    gb = lib.Bloom.create(gpu_ctx, len(path), 1e-3, k, threaded=True)
    gb.insert(path)
    # intercluster: only k-mers the path filter reports enter the table
    ot, gt = OrcTable(oracle, 2, k), lib.Table(gpu_ctx, 20_000, 2, k)
    for a, n, d in regions:
        ot.count_intercluster(ob, genome[a:a + n].tobytes(), d, 0 if d else 2, 0 if d else 1)
        gt.count_intercluster(gb, genome[a:a + n].tobytes(), d, 0 if d else 2, 0 if d else 1)
    wk, wm = _assert_tables_equal(gt, ot, "intercluster")
    assert len(wk) > 100 and (wm[:, 0] & 0x08).any() and (wm[:, 2] >= 4).any()     # path k-mers found, the decoy's and the repeat's among them
    ot.close(), gt.close()
    # parameter k-mers: the non-path k-mers, drawn per region
    seeds = [1234 + i for i in range(len(regions))]
    for fraction in (0.05, 1.0):
        ot, gt = OrcTable(oracle, 1, k), lib.Table(gpu_ctx, 40_000, 1, k)
        for (a, n, d), sd in zip(regions, seeds):
            ot.count_parameter_kmers(ob, genome[a:a + n].tobytes(), d, sd, fraction)
        gt.count_parameter_kmers(gb, genome.tobytes(), [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], seeds, fraction)
        wk, wm = _assert_tables_equal(gt, ot, f"parameter k-mers, fraction {fraction}")
        par, dec = (wm[:, 0] & 0x20) != 0, (wm[:, 0] & 0x08) != 0
        n_cand = sum(max(0, n - k + 1) for a, n, d in regions if not d)
        assert dec.sum() > 100 and (par.sum() > 0.9 * (n_cand - 1000) if fraction == 1.0 else 0.02 * n_cand < par.sum() < 0.08 * n_cand)
        ot.close(), gt.close()
    ob.close(), gb.close()
