"""getHaplotypeCandidates' bundle built and kept on the device (bt_paths_candidates_device) and handed to the sampler without a pass through the
host (bt_gibbs_source_create_from_paths), through the C ABI, against the oracle's bundle and the tests' own batch assembly.

With BT_PATHS_DEBUG set, bt_paths_candidates_device prints how many rows each of its three incidence kernels took (a lane per row up to 8
triples, a wavefront up to 64, a workgroup beyond: that one keeps the row's variants as a bit map over the 16-bit variant index, so it has no
row-length limit); BT_PATHS_ROW_LANE_MAX / BT_PATHS_ROW_WAVE_MAX lower the thresholds so that short rows reach the wider kernels too."""
import copy
import os
import re
import tempfile

import numpy as np
import pytest

import _oracle
from _gibbs_parity import assert_parity
from _oracle import OrcBloom, OrcGraphs, OrcKmc, OrcTable

pytestmark = pytest.mark.gpu

K = 55
ROW_FIELDS = ("hap_kmer_mult", "kmer_has_counts", "kmer_counts", "kmer_ic_mult", "kmer_shared", "kv_off", "kv_var", "kv_bits", "unique_idx", "multi_idx")


def _text(gs, first_path_only=False, every_path=False):
    nt = np.frombuffer(b"ACGT", np.uint8)
    if every_path:
        return np.concatenate([np.concatenate([nt[g.seq[v]] for v in range(len(g.seq)) if row[v]] + [np.frombuffer(b"N", np.uint8)]) for g in gs for row in g.paths])
    return np.concatenate([np.concatenate([nt[g.seq[v]] for v in range(len(g.seq)) if not first_path_only or g.paths[0, v]] + [np.frombuffer(b"N", np.uint8)]) for g in gs])


class Unit:
    """graphs + group structure + both sides' filters and tables, classified; `kmc`: counts through KMC databases (else the k-mers are inserted without counts)"""

    def __init__(self, ctx, oracle, gs, groups, S, rng, cluster_ids=None, sources=None, out_edges=None, excluded=(), kmc=True, in_table=None, full=(), classify=True):
        from bayestyper_amd import lib, synth_graphs

        self.ctx, self.oracle, self.gs, self.groups, self.S = ctx, oracle, gs, groups, S
        self.f = f = synth_graphs.flatten(gs)
        self.cluster_ids = list(range(len(gs))) if cluster_ids is None else cluster_ids
        self.sources = [list(range(len(g))) for g in groups] if sources is None else sources
        self.out_edges = [[] for _ in gs] if out_edges is None else out_edges
        self.gender = [s % 2 for s in range(S)]
        self.ploidy = np.full((len(groups), S), 2, np.uint8)
        self.og, self.gp = OrcGraphs(oracle, f, K), lib.Paths(ctx, f, K)
        n = int(f["seq_off"][-1]) * 4 + 100_000
        self.ob, self.gb = OrcBloom(oracle, n, 1e-3, K, threaded=True), lib.Bloom.create(ctx, n, 1e-3, K, threaded=True)
        self.og.count_kmers(self.ob)
        self.gp.count_kmers(self.gb)
        sel = gs if in_table is None else [gs[c] for c in in_table]
        km, va = oracle.kmers_from_sequence(_text(sel, first_path_only=kmc).tobytes(), K)
        if full:   # clusters with EVERY path k-mer in the table (with kmc, the others have those of their first path only)
            km2, va2 = oracle.kmers_from_sequence(_text([gs[c] for c in full], every_path=True).tobytes(), K)
            km, va = np.concatenate([km, km2]), np.concatenate([va, va2])
        present = np.unique(km[va == 1], axis=0)
        self.ot, self.gt = OrcTable(oracle, S, K), lib.Table(ctx, max(4 * len(present), 50_000), S, K)
        if kmc:
            with tempfile.TemporaryDirectory() as td:
                asc = oracle.unpack(present, K).reshape(-1, K)
                order = np.lexsort(asc.T[::-1])   # KMC order = ascending ASCII order
                for s in range(S):
                    cnt = rng.poisson(15, len(present)).astype(np.uint32) + 1
                    pref = os.path.join(td, f"s{s}")
                    oracle.kmc_write(pref, np.ascontiguousarray(asc[order]).reshape(-1), cnt[order], K, 3, 1)
                    db = OrcKmc(oracle, pref)
                    self.ot.parse_sample_kmers(self.ob, db, s)
                    sc = lib.KmcScan(ctx, db.k, db.p, db.counter_size, db.total, db.lut())
                    buf = ctx.to_device(db.payload())
                    sc.run(self.gb, self.gt, s, buf.ptr, 0, db.total)
                    ctx.sync()
                    sc.close(), buf.free(), db.close()
        else:
            self.ot.insert(oracle.unpack(present, K))
            self.gt.insert(present)
        # every k-mer of the `excluded` clusters is a multigroup k-mer: classified as excluded, so those clusters keep no row at all
        mg = np.zeros((0, 2), np.uint64)
        if excluded:
            km, va = oracle.kmers_from_sequence(_text([gs[c] for c in excluded], every_path=True).tobytes(), K)
            mg = np.unique(km[va == 1], axis=0)
        self.omg, self.gmg = OrcBloom(oracle, max(len(mg), 10), 1e-6, K), lib.Bloom.create(ctx, max(len(mg), 10), 1e-6, K, threaded=False)
        if len(mg):
            self.omg.insert(oracle.unpack(mg, K))
            self.gmg.insert(mg)
        if classify:
            n_o, ex_o = self.og.classify(self.ot, self.omg)
            n_g, ex_g = self.gp.classify(self.gt, self.gmg)
            assert np.array_equal(n_o, n_g) and np.array_equal(ex_o, ex_g)

    def expected(self):
        """the oracle's bundle and the batch the tests' own assembly makes of it"""
        from test_cli_gpu import _gibbs_batch

        co = self.og.candidates(self.ot)
        return co, _gibbs_batch(co, self.f, self.groups, self.S, self.ploidy, self.gender, self.cluster_ids, self.sources, self.out_edges)

    def structure(self, small):
        from bayestyper_amd import synth_graphs

        return synth_graphs.gibbs_structure(small, self.f, self.groups, self.S, self.gender, self.ploidy, self.cluster_ids, self.sources, self.out_edges)

    def device_source(self):
        from bayestyper_amd import lib

        sizes, small = self.gp.candidates_device(self.gt)
        return lib.GibbsSource.from_paths(self.ctx, self.gp, self.structure(small)), sizes

    def close(self):
        for x in (self.og, self.gp, self.ob, self.gb, self.ot, self.gt, self.omg, self.gmg):
            x.close()


def _row_triples(co, f):
    """per row of the oracle's bundle: the number of (variant, haplotype) incidences = sum of the popcounts of its entries' bitsets"""
    R = int(co["kmer_off"][-1])
    out = np.zeros(R, np.int64)
    at = 0
    for c in range(f["num_clusters"]):
        r0, r1 = int(co["kmer_off"][c]), int(co["kmer_off"][c + 1])
        e0, e1 = int(co["kv_off"][r0]), int(co["kv_off"][r1])
        hw = (int(f["num_paths"][c]) + 31) // 32
        if e1 > e0:
            bits = co["kv_bits"][at:at + (e1 - e0) * hw].reshape(e1 - e0, hw)
            pop = np.unpackbits(bits.view(np.uint8), axis=1).sum(axis=1)
            row_of = np.repeat(np.arange(r0, r1), np.diff(co["kv_off"][r0:r1 + 1].astype(np.int64)))
            np.add.at(out, row_of, pop)
        at += (e1 - e0) * hw
    return out


def _debug_line(err):
    lines = [ln for ln in err.splitlines() if ln.startswith("bt_paths_candidates: rows=")]
    assert lines, err
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[-1])}


def _mixed_unit(ctx, oracle, S, seed):
    """SNV / indel / multi-allelic clusters; a group of three clusters over the same sequence (two of them with the same paths: only multicluster rows);
    clusters with > 32, > 64 and > 256 paths; a parent with a nested child in its group; a cluster whose k-mers are all excluded (no row, no entry)"""
    from bayestyper_amd import synth_graphs

    rng = np.random.default_rng(seed)
    gs = [synth_graphs.random_cluster(rng, K, int(rng.integers(1, 5)), int(rng.integers(2, 8))) for _ in range(6)]
    a = synth_graphs.random_cluster(rng, K, 3, 6)
    b = copy.deepcopy(a)                                   # same sequence, same paths: every row of both is a multicluster row
    c = copy.deepcopy(a)
    c.paths = synth_graphs.random_paths(c, rng, 3)         # same sequence, other paths
    wide = [synth_graphs.random_cluster(rng, K, 8, 40, kinds=("snv", "multi")), synth_graphs.random_cluster(rng, K, 9, 70, kinds=("snv", "ins")),
            synth_graphs.random_cluster(rng, K, 11, 800, kinds=("snv",))]
    parent = synth_graphs.random_cluster(rng, K, 4, 5, nested_cluster=900)
    child = synth_graphs.random_cluster(rng, K, 2, 3)
    gone = synth_graphs.random_cluster(rng, K, 2, 3)
    clusters = gs[:3] + [a, b, c] + wide + [parent, child, gone] + gs[3:]
    ia, ip, ig = 3, 9, 11
    groups = [[0], [1], [2], [ia, ia + 1, ia + 2], [6], [7], [8], [ip, ip + 1], [ig]] + [[i] for i in range(12, len(clusters))]
    ids = list(range(100, 100 + len(clusters)))
    ids[ip + 1] = 900
    sources = [[0] if g == [ip, ip + 1] else list(range(len(g))) for g in groups]
    edges = [[] for _ in clusters]
    edges[ip] = [1]
    in_table = [i for i in range(len(clusters)) if i != 0]   # cluster 0: no k-mer in the table, so no multicluster row and no counts
    return Unit(ctx, oracle, clusters, groups, S, rng, cluster_ids=ids, sources=sources, out_edges=edges, excluded=[ig], in_table=in_table, full=[ia, ia + 1, ig])


def _compare(expected, got, what):
    from bayestyper_amd import lib

    for name, _ in lib.SOURCE_FIELDS:
        assert np.array_equal(np.asarray(expected[name]).reshape(-1), got[name]), f"{what}: {name}"


@pytest.mark.parametrize("S,seed", [(1, 11), (3, 12), (10, 13)])
def test_source_arrays_equal_oracle(gpu_ctx, oracle, monkeypatch, capfd, S, seed):
    """the device-built source, field by field, equals the batch made of the ORACLE's bundle; the same source as the host route gives; three builds of the
    same unit give identical arrays; every incidence kernel is reached, at the default thresholds and at lowered ones"""
    from bayestyper_amd import lib, synth_graphs

    u = _mixed_unit(gpu_ctx, oracle, S, seed)
    co, exp = u.expected()
    f, koff, moff, uoff = u.f, co["kmer_off"].astype(np.int64), co["multi_off"].astype(np.int64), co["unique_off"].astype(np.int64)
    # the unit holds what it was built to hold (asserted on the oracle's bundle)
    trip = _row_triples(co, f)
    assert trip.max() > 256 and ((trip > 8) & (trip <= 64)).any() and (trip <= 8).any(), trip.max()
    assert (f["num_paths"] > 64).any() and ((f["num_paths"] > 32) & (f["num_paths"] <= 64)).any()
    K_c, M_c = np.diff(koff), np.diff(moff)
    assert ((M_c == 0) & (K_c > 0)).any() and ((M_c == K_c) & (K_c > 0)).any() and (K_c == 0).any()       # no multicluster rows / only such rows / no row, no entry
    assert len(co["hapnest_idx"]) > 0 and len(co["nestdep_var"]) > 0
    g3 = next(g for g in u.groups if len(g) >= 3)
    sh = [exp["kmer_shared"][koff[c]:koff[c + 1]] for c in g3]
    assert all((x >= 0).any() for x in sh) and len(set(sh[0][sh[0] >= 0]) & set(sh[1][sh[1] >= 0]) & set(sh[2][sh[2] >= 0])) > 0   # one record shared by three clusters
    assert exp["group_num_shared"][u.groups.index(g3)] < sum(int((x >= 0).sum()) for x in sh)
    # 2. the host route: bt_paths_candidates + fetch -> batch -> source
    cg = u.gp.candidates(u.gt)
    for name in co:
        assert np.array_equal(co[name], cg[name]), name
    flat_host = synth_graphs.gibbs_batch_from_candidates(cg, f, u.groups, S, u.gender, u.ploidy, u.cluster_ids, u.sources, u.out_edges)
    host = lib.GibbsSource.from_batch(gpu_ctx, flat_host)
    host_arrays, host_bytes = host.fetch(), host.device_bytes()
    host.close()
    _compare(exp, host_arrays, "host route")
    # 1. + 3. the device route, three times at the default thresholds, then with thresholds that send short rows to the wider kernels
    monkeypatch.setenv("BT_PATHS_DEBUG", "1")
    for rep, (lane_max, wave_max) in enumerate([(None, None), (None, None), (None, None), (2, 6), (0, 0)]):
        for name, v in (("BT_PATHS_ROW_LANE_MAX", lane_max), ("BT_PATHS_ROW_WAVE_MAX", wave_max)):
            monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, str(v))
        capfd.readouterr()
        src, sizes = u.device_source()
        dbg = _debug_line(capfd.readouterr().err)
        got = src.fetch()
        _compare(exp, got, f"device route, build {rep}")
        for name in got:
            assert np.array_equal(got[name], host_arrays[name]), name
        assert src.device_bytes() == host_bytes
        src.close()
        lm, wm = (8, 64) if lane_max is None else (lane_max, wave_max)
        assert dbg["lane_max"] == lm and dbg["wave_max"] == wm and dbg["rows"] == koff[-1] == sizes["rows"]
        assert dbg["lane_rows"] + dbg["wave_rows"] + dbg["block_rows"] == dbg["rows"] and dbg["longest_row"] >= trip.max() and dbg["triples"] >= trip.sum()
        # a row's triples are at least its distinct incidences (a k-mer seen twice on a path repeats one)
        assert dbg["block_rows"] >= (trip > wm).sum() >= 1 and dbg["lane_rows"] <= (trip <= lm).sum()
        if lane_max is None or lane_max == 2:
            assert dbg["wave_rows"] >= 1 and dbg["lane_rows"] >= 1
        else:
            assert dbg["wave_rows"] == 0 and dbg["block_rows"] == (trip > 0).sum()    # every row with an incidence went through the workgroup kernel
    u.close()


def test_large_unit_multi_block_scans(gpu_ctx, oracle):
    """>= 20 000 clusters: every prefix sum (rows, triples, entries, multicluster rows, shared records) runs over many blocks"""
    from bayestyper_amd import synth_graphs

    rng = np.random.default_rng(21)
    base = [synth_graphs.random_cluster(rng, K, int(rng.integers(1, 4)), int(rng.integers(2, 5)), kinds=("snv", "ins", "del")) for _ in range(250)]
    gs = [base[i % len(base)] for i in range(20_000 + 17)]
    groups, at = [], 0
    while at < len(gs):        # groups of 1 .. 4 clusters; a group may hold the same base cluster twice only when it spans a multiple of 250, never here
        n = min(int(rng.integers(1, 5)), len(gs) - at)
        groups.append(list(range(at, at + n)))
        at += n
    u = Unit(gpu_ctx, oracle, gs, groups, 2, rng, kmc=False, in_table=list(range(40)))
    co, exp = u.expected()
    assert co["kmer_off"][-1] > 4 * 1024 and len(co["multi_idx"]) > 4 * 1024 and co["kv_off"][-1] > 4 * 1024 and exp["group_num_shared"].sum() > 4 * 1024
    src, sizes = u.device_source()
    _compare(exp, src.fetch(), "large unit")
    src.close()
    u.close()


def _subset(r, goff, ids):
    cl = [c for g in ids for c in range(int(goff[g]), int(goff[g + 1]))]
    d = [(int(r["dip_off"][c]), int(r["dip_off"][c + 1])) for c in cl]
    e = [(int(r["cell_off"][c]), int(r["cell_off"][c + 1])) for c in cl]
    cat = lambda a, se: np.concatenate([a[s:t] for s, t in se]) if se else a[:0]
    return {"dip_off": np.concatenate([[0], np.cumsum([t - s for s, t in d])]).astype(np.uint64), "h1": cat(r["h1"], d), "h2": cat(r["h2"], d), "freq": cat(r["freq"], d),
            "cell_off": np.concatenate([[0], np.cumsum([t - s for s, t in e])]).astype(np.uint64), "stats": cat(r["stats"], e)}


@pytest.mark.parametrize("noise_seeding", [0, 1])
def test_samplers_from_device_source_match_oracle(gpu_ctx, oracle, noise_seeding):
    """samplers over all groups, a shuffled subset and two consecutive ranges of the device-built source: per group the oracle's trace and results"""
    S, TR = 2, 12
    u = _mixed_unit(gpu_ctx, oracle, S, 31)
    co, exp = u.expected()
    kw = dict(seed=5, chains=2, burn=8, iters=20, noise_seeding=noise_seeding)
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    og = _oracle.OrcGibbs(oracle, exp, lut_g, lut_n, **kw)
    og.trace_enable(TR)
    og.run(8)
    ro = og.results()
    goff, G = exp["group_cluster_off"], exp["num_groups"]
    tro = [og.trace(g, int(goff[g + 1] - goff[g]), TR) for g in range(G)]
    og.close()
    src, _ = u.device_source()
    perm = np.random.default_rng(3).permutation(G)
    for ids in (None, perm[: G // 2 + 1], np.arange(0, G // 2), np.arange(G // 2, G)):
        gg = src.sampler(kw, ids, lut_g, lut_n)
        gg.trace_enable(TR)
        gg.run()
        gpu_ctx.sync()
        rg, trg = gg.results(), gg.trace()
        sel = list(range(G)) if ids is None else [int(i) for i in ids]
        for i, g in enumerate(sel):
            assert np.array_equal(tro[g], trg[i][: len(tro[g])]), f"group {g}"
        assert_parity({"S": S, "num_clusters": sum(int(goff[g + 1] - goff[g]) for g in sel)}, _subset(ro, goff, sel), rg, 2 * 20)
        gg.close()
    src.close()
    u.close()


def test_errors_leave_nothing_allocated(gpu_ctx, oracle):
    from bayestyper_amd import lib, synth_graphs

    rng = np.random.default_rng(41)
    gs = [synth_graphs.random_cluster(rng, K, 2, 3) for _ in range(4)]
    big = synth_graphs.random_cluster(rng, K, 1, 2, chrom_len=1200)
    big.seq[-1] = np.concatenate([big.seq[-1], np.zeros(300, np.uint8)])    # a homopolymer: one k-mer 246 times on a path
    groups = [[0, 1], [2], [3]]
    u = Unit(gpu_ctx, oracle, gs, groups, 2, rng, kmc=False)
    cg = u.gp.candidates(u.gt)

    def fails(fn, match):
        gpu_ctx.sync()
        before = gpu_ctx.info()["hbm_free"]
        with pytest.raises(lib.BtError, match=match):
            fn()
        gpu_ctx.sync()
        assert gpu_ctx.info()["hbm_free"] == before, match

    st0 = u.structure({n: cg[n] for n in lib.Paths._SMALL})
    # the bundle is on the host (bt_paths_candidates): nothing on the device for a source to take
    fails(lambda: lib.GibbsSource.from_paths(gpu_ctx, u.gp, st0), "no candidates on the device")
    sizes, small = u.gp.candidates_device(u.gt)
    good = u.structure(small)
    gpu_ctx.sync()
    held = gpu_ctx.info()["hbm_free"]
    bad = dict(good, num_clusters=len(gs) - 1)
    fails(lambda: lib.GibbsSource.from_paths(gpu_ctx, u.gp, bad), "number of clusters")
    bad = dict(good, num_haplotypes=good["num_haplotypes"] + np.uint32(1))
    fails(lambda: lib.GibbsSource.from_paths(gpu_ctx, u.gp, bad), "num_haplotypes")
    bad = dict(good, kv_off=np.zeros(sizes["rows"] + 1, np.uint32))
    fails(lambda: lib.GibbsSource.from_paths(gpu_ctx, u.gp, bad), "must be NULL")
    out = lib._CandOut()
    out.kmer_counts = np.zeros(8, np.uint8).ctypes.data
    assert lib.bt_paths_candidates_fetch_small(u.gp.h, lib.C.byref(out)) != 0 and b"must be NULL" in lib.bt_last_error()
    src = lib.GibbsSource.from_paths(gpu_ctx, u.gp, good)      # after the refused calls the handle still holds its candidates
    fails(lambda: lib.GibbsSource.from_paths(gpu_ctx, u.gp, good), "no candidates on the device")   # a second source from the same candidates
    src.close()
    gpu_ctx.sync()
    assert gpu_ctx.info()["hbm_free"] >= held     # the source released what it took
    u.close()
    # a k-mer more than 127 times on one haplotype that is not an excluded k-mer (nothing classified it): an error of the call
    u2 = Unit(gpu_ctx, oracle, gs + [big], groups + [[4]], 2, rng, kmc=False, classify=False)
    sz = lib._CandSizes()
    lib.bt_paths_candidates_device(u2.gp.h, u2.gt.h, lib.C.byref(sz))     # (first call: builds the handle's index, which it keeps)
    fails(lambda: lib.check(lib.bt_paths_candidates_device(u2.gp.h, u2.gt.h, lib.C.byref(sz))), "more than 127 times")
    fails(lambda: lib.GibbsSource.from_paths(gpu_ctx, u2.gp, good), "no candidates on the device")
    u2.close()
