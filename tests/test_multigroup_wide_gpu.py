"""GPU tests of the workgroup route of the multigroup pass (mg_order_wide_kernel, BT_MG_WIDE_MIN): the device's k-mer-set orders against the
real container of the reference (oracle/_ref/libbtref.so), and the pass itself against the oracle with the route switched on."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mg_wide_groups as MG  # noqa: E402
from _oracle import OrcBloom, OrcGraphs, OrcTable  # noqa: E402

pytestmark = pytest.mark.gpu
K = MG.K


def _sorted_export(kmers, counts, meta):
    order = np.lexsort((kmers[:, 0], kmers[:, 1]))
    return kmers[order], counts[order], meta[order]


def test_kmer_set_orders_on_device(gpu_ctx, oracle, ref):
    """bt_kmer_set_orders (the routine steps 2 and 3 of bt_paths_count_multigroup run) over the group sequence of the CPU test, with every
    group on a lane (wide_min 0), every non-empty group on a workgroup (1), and mixed (64, 5000): ranks and bucket counts equal the real
    container's for every threshold, hence one another; num_wide_groups counts the groups of at least wide_min k-mers.  In the sequence the
    70 000 group inherits 42 043 buckets and has two stages, so it is also ordered alone in a fresh set: 13 stages, the order again the
    real container's."""
    from bayestyper_amd import lib

    seq = MG.group_sequence(oracle, ref)
    sizes = [len(p) for p in seq["packed"]]
    for wide_min in (0, 1, 64, 5000):
        ranks, final, stats = lib.kmer_set_orders(gpu_ctx, seq["packed"], K, 1, wide_min)
        for g, rank in enumerate(ranks):
            assert np.array_equal(MG.order_of(rank), seq["order"][g]), f"wide_min {wide_min}, group {g} ({sizes[g]} k-mers)"
        assert np.array_equal(final, seq["buckets"]), wide_min
        want_wide = sum(1 for n in sizes if wide_min and n >= max(wide_min, 1))
        assert stats["num_groups"] == len(sizes) and stats["num_wide_groups"] == want_wide and stats["wide_min_kmers"] == wide_min
        assert stats["max_group_kmers"] == 70000
        assert (stats["wide_scratch_bytes"] > 0) == (want_wide > 0)
        assert stats["max_stages"] == (4 if wide_min else 0)   # 700 from 127 buckets, 30 000 from 5 087: four stages each
        if wide_min:   # the 70 000 group is wide for each of these thresholds
            ranks, final, stats = lib.kmer_set_orders(gpu_ctx, [seq["packed"][MG.BIG]], K, 1, wide_min)
            assert np.array_equal(MG.order_of(ranks[0]), seq["fresh_order"]) and int(final[0]) == seq["fresh_buckets"]
            assert stats["num_wide_groups"] == 1 and stats["max_stages"] >= 10


def _two_units(gpu_ctx, oracle, n_filter, fpr, threaded):
    """the construction of test_kmer_gpu.py::test_path_multigroup_kmers: two units sharing filter and table, groups of very different sizes;
    table, num_path_kmers and sampled filter words must equal the oracle's.  Returns bt_paths_multigroup_info of each unit."""
    from bayestyper_amd import lib, synth_graphs

    rng = np.random.default_rng(41)
    ob = OrcBloom(oracle, n_filter, fpr, K, threaded=threaded)
    gb = lib.Bloom.create(gpu_ctx, n_filter, fpr, K, threaded=threaded)
    ot, gt = OrcTable(oracle, 1, K), lib.Table(gpu_ctx, 16 if fpr > 1e-3 else 200_000, 1, K)
    shared = None
    total = 0
    infos = []
    for unit in range(2):
        sizes = [int(rng.integers(1, 5)) for _ in range(12)] + [40, 1, 2, 90, 3]      # variants per cluster: small groups after large ones
        gs = [synth_graphs.random_cluster(rng, K, v, int(rng.integers(2, 7))) for v in sizes]
        gs[3] = copy.deepcopy(gs[2])     # same group as 2 -> shared k-mers are NOT multigroup
        gs[3].paths = synth_graphs.random_paths(gs[3], rng, 3)
        gs[9] = copy.deepcopy(gs[5])     # different group -> multigroup
        gs[9].paths = synth_graphs.random_paths(gs[9], rng, 2)
        if unit == 0:
            shared = copy.deepcopy(gs[7])
        else:
            gs[1] = shared               # a cluster of the previous unit: its k-mers are in the filter already
        f = synth_graphs.flatten(gs)
        cluster_group = np.array([0, 1, 2, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, 11, 11, 12, 13], np.uint32)
        og, gp = OrcGraphs(oracle, f, K), lib.Paths(gpu_ctx, f, K)
        n_o = og.count_multigroup(cluster_group, ob, ot)
        n_g = gp.count_multigroup(cluster_group, gb, gt)
        infos.append(gp.multigroup_info())
        assert n_o == n_g and n_o > 0
        total += n_o
        gk, _, _ = _sorted_export(*gt.export())
        wk, _, _ = _sorted_export(*ot.export())
        assert len(wk) > 50 and np.array_equal(gk, wk), (unit, len(gk), len(wk))
        for sub in (range(0, 65536, 4099) if threaded else [0]):
            assert np.array_equal(gb.bits(sub), ob.bits(sub))
        og.close(), gp.close()
    if fpr > 1e-3:   # the undersized filters: most multigroup entries are false positives of the moment, i.e. the order is visible
        assert len(wk) > 0.02 * total
    for x in (ob, gb, ot, gt):
        x.close()
    return infos


@pytest.mark.parametrize("wide_min", [1, 64, 1000])
@pytest.mark.parametrize("n_filter,fpr,threaded", [(1_000_000, 1e-7, True), (3000, 0.02, False), (20000, 0.01, True)])
def test_path_multigroup_kmers_wide_route(gpu_ctx, oracle, monkeypatch, n_filter, fpr, threaded, wide_min):
    """countPathMultigroupKmers with BT_MG_WIDE_MIN = 1 (every group on a workgroup), 64 and 1000: the pass equals the oracle's, which runs the
    reference's loop on the real container; with the undersized filters a wrong order would change which k-mers are false positives of the
    moment.  Every unit has a wide group.  In this construction even a group of one single-variant cluster has more than 64 distinct k-mers
    (k = 55: measured on the device, 14 wide groups of 14 with 64), so the mixed case — some groups on a workgroup, at least one left on the lane
    route — is the threshold 1000: the groups of 40 and 90 variants have thousands of k-mers, a group of one single-variant cluster (at most six
    alleles of about a hundred windows) stays below it."""
    monkeypatch.setenv("BT_MG_WIDE_MIN", str(wide_min))
    for info in _two_units(gpu_ctx, oracle, n_filter, fpr, threaded):
        assert info["num_groups"] == 14 and info["wide_min_kmers"] == wide_min
        assert info["num_wide_groups"] >= 1 and info["wide_scratch_bytes"] > 0 and info["max_stages"] >= 1
        assert info["max_group_kmers"] >= 1000
        if wide_min in (1, 64):   # (every group of the construction has more than 64 distinct k-mers)
            assert info["num_wide_groups"] == info["num_groups"]
        if wide_min == 1000:
            assert info["num_wide_groups"] < info["num_groups"]


def test_switch_unset_is_the_lane_route(gpu_ctx, oracle, monkeypatch):
    """BT_MG_WIDE_MIN unset: no wide group, no work area — the lane route for every group, as before the switch existed"""
    monkeypatch.delenv("BT_MG_WIDE_MIN", raising=False)
    for info in _two_units(gpu_ctx, oracle, 3000, 0.02, False):
        assert info["num_groups"] == 14 and info["num_wide_groups"] == 0 and info["wide_scratch_bytes"] == 0
        assert info["wide_min_kmers"] == 0 and info["max_stages"] == 0 and info["max_group_kmers"] > 0


def test_malformed_switch_fails_the_call(gpu_ctx, oracle, monkeypatch):
    """BT_MG_WIDE_MIN must be a decimal number below 2^32: anything else fails bt_paths_count_multigroup with a message instead of becoming some
    threshold, and bt_paths_multigroup_info keeps describing the last call that succeeded (none here: all zero)"""
    from bayestyper_amd import lib, synth_graphs

    rng = np.random.default_rng(5)
    f = synth_graphs.flatten([synth_graphs.random_cluster(rng, K, 2, 3) for _ in range(3)])
    gb = lib.Bloom.create(gpu_ctx, 10000, 1e-3, K, threaded=False)
    gt = lib.Table(gpu_ctx, 1000, 1, K)
    gp = lib.Paths(gpu_ctx, f, K)
    for bad in ("-1", "abc", "12x", "4294967296", ""):
        monkeypatch.setenv("BT_MG_WIDE_MIN", bad)
        with pytest.raises(lib.BtError, match="BT_MG_WIDE_MIN"):
            gp.count_multigroup(np.arange(3, dtype=np.uint32), gb, gt)
        assert gp.multigroup_info()["num_groups"] == 0
    monkeypatch.setenv("BT_MG_WIDE_MIN", "1")
    assert gp.count_multigroup(np.arange(3, dtype=np.uint32), gb, gt) > 0
    assert gp.multigroup_info()["num_wide_groups"] == 3
    for x in (gp, gb, gt):
        x.close()
