"""A sample scan sharded over W ranks, emulated on one GPU through the C ABI: every rank scans its record slice of every sample's KMC database
(bt_kmc_scan_run_file / bt_kmc_scan_run_host with first_record != 0 and n < total, as KmerCounter::parseSampleKmers passes them), exports its count
rows and merges the rows of the other ranks.  Every rank's table must then equal the oracle's one-rank table (OrcTable.parse_sample_kmers over whole
databases), exactly.  A database scanned with a counter range is compared with the oracle's scan of a database that holds the in-range records only
(the oracle's reader knows no range; test_kmer_gpu.py::test_kmc_counter_range_filter compares the same way)."""
import numpy as np
import pytest

import _oracle
from _oracle import OrcBloom, OrcKmc, OrcTable

K = 55
S = 5
# (records drawn, LUT prefix length, counter bytes, KMC2 bins or 0 for the KMC1 layout, counter range or None): record bytes 13, 15, 13, 12, 13
SAMPLES = [(20_000, 7, 1, 0, (3, 250)), (9_001, 3, 2, 0, None), (15_000, 7, 1, 6, (2, 249)), (7_003, 11, 1, 0, None), (2, 7, 1, 0, None)]
WORLDS = [1, 2, 3, 5]


def _slice(total, world, rank):
    """KmerCounter::parseSampleKmers: rank r of w scans records [first, first + count)"""
    return total // world * rank + min(rank, total % world), total // world + (1 if rank < total % world else 0)


def _sorted(kmers, counts, meta):
    order = np.lexsort((kmers[:, 0], kmers[:, 1]))
    return kmers[order], counts[order], meta[order]


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_sorted(*a), _sorted(*b)))


def _flat(a):
    return np.ascontiguousarray(a).reshape(-1)


@pytest.fixture(scope="module")
def shards(oracle, tmp_path_factory):
    """the databases, the path Bloom's members, the parameter k-mers and the oracle's one-rank results (CPU only; computed once)"""
    tmp = tmp_path_factory.mktemp("sharded_scan")
    rng = np.random.default_rng(2024)
    # the pool the samples draw from: the canonical k-mers of a random sequence
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 32_000 + K - 1)].tobytes()
    km, valid = oracle.kmers_from_sequence(seq, K)
    pool = np.unique(oracle.unpack(km[valid == 1], K).reshape(-1, K), axis=0)   # sorted ascending: KMC order
    assert len(pool) >= 31_000
    dbs, path = [], []
    for s, (n, p, cs, bins, crange) in enumerate(SAMPLES):
        sel = pool[np.sort(rng.choice(len(pool), n, replace=False))]
        counts = rng.integers(1, 256, n).astype(np.uint32)
        prefix = str(tmp / f"s{s}")
        write = (lambda pre, k_, c_: oracle.kmc2_write(pre, _flat(k_), c_, K, p, cs, bins)) if bins else (lambda pre, k_, c_: oracle.kmc_write(pre, _flat(k_), c_, K, p, cs))
        write(prefix, sel, counts)
        ref_prefix = prefix
        if crange:   # what the oracle reads instead: the records a reader with this counter range returns
            keep = (counts >= crange[0]) & (counts <= crange[1])
            assert 0 < (~keep).sum() < n // 10
            ref_prefix = prefix + "_inrange"
            write(ref_prefix, sel[keep], counts[keep])
        db = OrcKmc(oracle, prefix)
        assert (db.total, db.rec_size) == (n, (K - p) // 4 + cs)
        dbs.append({"prefix": prefix, "ref_prefix": ref_prefix, "p": p, "cs": cs, "bins": bins, "range": crange, "total": db.total, "rec": db.rec_size, "lut": db.lut(),
                    "payload": db.payload(), "suf": prefix + ".kmc_suf"})
        db.close()
        path.append(sel[rng.choice(n, min(n, 1500), replace=False)])
    path = np.unique(np.concatenate(path), axis=0)
    param = np.concatenate([pool[rng.choice(len(pool), 150, replace=False)],
                            _oracle.canonical_ascii(oracle, _oracle.random_kmers(rng, 150, K), K).reshape(-1, K)])
    param = np.unique(param, axis=0)
    ob = OrcBloom(oracle, len(path), 1e-2, K, threaded=True)
    ob.insert(_flat(path))
    ot = OrcTable(oracle, S, K)
    ot.insert(_flat(param), mark_parameter=True)
    one = OrcTable(oracle, 1, K)   # sample 0 alone, into an empty table
    hits = []
    for s, d in enumerate(dbs):
        db = OrcKmc(oracle, d["ref_prefix"])
        hits.append(ot.parse_sample_kmers(ob, db, s))
        if s == 0:
            assert one.parse_sample_kmers(ob, db, 0) == hits[0]
        db.close()
    want, want_one = _sorted(*ot.export()), _sorted(*one.export())
    for x in (ob, ot, one):
        x.close()
    return {"dbs": dbs, "path": oracle.pack(_flat(path), K), "param": oracle.pack(_flat(param), K), "want": want, "hits": hits, "want_one": want_one}


def test_the_inputs_hold_the_edges(shards):
    """what the slices of WORLDS and the oracle's table must contain for the scans below to mean something (asserted on the inputs alone; needs no GPU)"""
    dbs = shards["dbs"]
    slices = [(d, w, r) + _slice(d["total"], w, r) for d in dbs for w in WORLDS for r in range(w)]
    for d in dbs:
        for w in WORLDS:
            parts = [_slice(d["total"], w, r) for r in range(w)]
            assert parts[0][0] == 0 and sum(n for _, n in parts) == d["total"] and all(parts[r][0] + parts[r][1] == parts[r + 1][0] for r in range(w - 1))
    assert sum(1 for d, w, r, first, n in slices if n == 0) >= 2                                      # the two-record sample, W = 3 and W = 5
    assert any(first % 2 == 1 and (first * d["rec"]) % 16 != 0 and n > 0 for d, w, r, first, n in slices)
    assert any(first % 16 != 0 and n > 1024 for d, w, r, first, n in slices)                          # (an odd start with several 1024-record routed chunks)
    kmc2 = [d for d in dbs if d["bins"]]
    assert len(kmc2) == 1 and len(kmc2[0]["lut"]) == kmc2[0]["bins"] * 4 ** kmc2[0]["p"] + 1
    bin_start = kmc2[0]["lut"][::4 ** kmc2[0]["p"]][:-1].astype(np.int64)
    assert (np.diff(bin_start) > 1000).all()
    inside = [first for d, w, r, first, n in slices if d is kmc2[0] and n > 0 and first > bin_start[1] and first not in bin_start]
    crossing = [first for d, w, r, first, n in slices if d is kmc2[0] and ((bin_start > first) & (bin_start < first + n)).any()]
    assert inside and crossing                                                                        # a start inside a later bin; a slice across a bin boundary
    wk = shards["want"][0]
    known = {tuple(x) for x in shards["path"].tolist()} | {tuple(x) for x in shards["param"].tolist()}
    false_positives = sum(1 for x in wk.tolist() if tuple(x) not in known)
    assert false_positives >= 10, false_positives
    assert (shards["want"][1] != 0).any(1).sum() > 5000 and all(h > 0 for h in shards["hits"][:4])


@pytest.fixture(scope="module")
def path_bloom(gpu_ctx, shards):
    from bayestyper_amd import lib

    gb = lib.Bloom.create(gpu_ctx, len(shards["path"]), 1e-2, K, threaded=True)
    gb.insert(shards["path"])
    yield gb
    gb.close()


def _scan(lib, ctx, d):
    sc = lib.KmcScan(ctx, K, d["p"], d["cs"], d["total"], d["lut"])
    if d["range"]:
        sc.set_count_range(*d["range"])
    return sc


def _run(sc, d, mode, bloom, table, s, first, n, chunk):
    if mode == "file":
        return sc.run_file(bloom, table, s, d["suf"], first, n, chunk)
    return sc.run_host(bloom, table, s, d["payload"][first * d["rec"]:], first, n, chunk)   # h_records points at record `first` (KmcFile.cpp:119)


@pytest.mark.gpu
# chunk_records 1000 is rounded down to 992 inside; 16 is the smallest; 0 = the default (one chunk here)
@pytest.mark.parametrize("world,mode,chunk,routed", [(1, "file", 0, "0"), (1, "host", 1000, "1"), (2, "file", 16, "1"), (2, "host", 0, "0"), (3, "file", 1000, "1"),
                                                     (3, "host", 16, "0"), (5, "file", 0, "1"), (5, "file", 1000, "0"), (5, "host", 16, "1")])
def test_ranks_scan_slices_and_merge(gpu_ctx, shards, path_bloom, monkeypatch, world, mode, chunk, routed):
    from bayestyper_amd import lib

    monkeypatch.setenv("BT_KMC_ROUTED", routed)
    tables, exported = [], []
    try:
        for r in range(world):
            t = lib.Table(gpu_ctx, 20_000, S, K)
            tables.append(t)
            t.insert(shards["param"], mark_parameter=True)
        hits = [0] * S
        for s, d in enumerate(shards["dbs"]):
            for r in range(world):
                first, n = _slice(d["total"], world, r)
                sc = _scan(lib, gpu_ctx, d)   # (a handle per rank and sample, as parseSampleKmers creates them)
                hits[s] += _run(sc, d, mode, path_bloom, tables[r], s, first, n, chunk)
                sc.close()
        assert hits == shards["hits"]
        exported = [t.export_count_rows() for t in tables]
        for r, t in enumerate(tables):
            for o, (buf, n) in enumerate(exported):
                if o != r and n:
                    t.merge_count_rows(buf, n)
        gpu_ctx.sync()
        for r, t in enumerate(tables):
            assert not t.status()["overflowed"]
            assert _equal(t.export(), shards["want"]), f"rank {r} of {world}"
    finally:
        for buf, _ in exported:
            buf.free()
        for t in tables:
            t.close()


@pytest.mark.gpu
def test_staging_regrown_then_handed_on(shards, monkeypatch):
    """One handle, three run_file calls with chunks of 16, 4096 and 16 records: the staging buffers are regrown (the small ones go to the context), then
    reused as they are.  Destroying the handle leaves the large ones with the context; a second handle scanning with chunks of 1000 takes them from
    there.  On a context of its own, so that which branch runs does not depend on the tests before."""
    from bayestyper_amd import lib

    monkeypatch.setenv("BT_KMC_ROUTED", "0")
    d = shards["dbs"][0]
    ctx = lib.Ctx(0)
    bloom = lib.Bloom.create(ctx, len(shards["path"]), 1e-2, K, threaded=True)
    bloom.insert(shards["path"])
    tables = []
    try:
        sc = _scan(lib, ctx, d)
        for chunk in (16, 4096, 16):
            tables.append(lib.Table(ctx, 20_000, 1, K))
            assert sc.run_file(bloom, tables[-1], 0, d["suf"], 0, d["total"], chunk) == shards["hits"][0]
        sc.close()
        sc = _scan(lib, ctx, d)
        tables.append(lib.Table(ctx, 20_000, 1, K))
        assert sc.run_file(bloom, tables[-1], 0, d["suf"], 0, d["total"], 1000) == shards["hits"][0]
        sc.close()
        for i, t in enumerate(tables):
            assert _equal(t.export(), shards["want_one"]), i
    finally:
        for t in tables:
            t.close()
        bloom.close()
        ctx.close()


@pytest.mark.gpu
def test_scan_errors_are_reported(gpu_ctx, shards, path_bloom, tmp_path):
    """ordinary error returns with bt_last_error text; the handle and the table stay usable"""
    from bayestyper_amd import lib

    d = shards["dbs"][0]
    t = lib.Table(gpu_ctx, 20_000, 1, K)
    sc = _scan(lib, gpu_ctx, d)
    try:
        with pytest.raises(lib.BtError, match="record range exceeds"):
            sc.run_file(path_bloom, t, 0, d["suf"], d["total"] - 10, 11)
        with pytest.raises(lib.BtError, match="record range exceeds"):
            sc.run_host(path_bloom, t, 0, d["payload"], d["total"] - 10, 11)
        with pytest.raises(lib.BtError, match="cannot open"):
            sc.run_file(path_bloom, t, 0, str(tmp_path / "missing.kmc_suf"), 0, d["total"])
        # a .kmc_suf that ends one record early: the read of the last chunk fails
        short = str(tmp_path / "short.kmc_suf")
        with open(d["suf"], "rb") as f:
            whole = f.read()
        assert len(whole) == 8 + d["total"] * d["rec"]
        with open(short, "wb") as f:
            f.write(whole[:4 + (d["total"] - 1) * d["rec"]])
        with pytest.raises(lib.BtError, match="reading the records failed"):
            sc.run_file(path_bloom, t, 0, short, d["total"] - 100, 100)
        assert t.status()["num_keys"] == 0 and not t.status()["overflowed"]
        # n = 0: no hits, nothing touched (not even the file)
        assert sc.run_file(path_bloom, t, 0, d["suf"], d["total"], 0) == 0 and sc.run_host(path_bloom, t, 0, d["payload"], 7, 0) == 0
        assert t.status()["num_keys"] == 0
        # and the handle still scans
        assert sc.run_file(path_bloom, t, 0, short, 0, d["total"] - 1) + sc.run_host(path_bloom, t, 0, d["payload"][(d["total"] - 1) * d["rec"]:], d["total"] - 1, 1) == shards["hits"][0]
        assert _equal(t.export(), shards["want_one"])
    finally:
        sc.close()
        t.close()
