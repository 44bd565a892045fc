"""getKmerStats on the GPU (bt_kmc_scan_kmer_stats*, the `getKmerStats` executable) against the reference's own listing: the expected
histogram is CKMCFile::ReadNextKmer's listing (oracle/_ref: ref_kmc_list, count-range filter included) with each k-mer's letters counted,
which is getKmerStats.cpp:87-127's loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _oracle  # noqa: E402
from _oracle import OrcKmc  # noqa: E402
from test_kmer_stats_cpu import HEADER, expected_hist, kmc_count_range, kmc_patch, run_exe  # noqa: E402

pytestmark = pytest.mark.gpu
K = 55


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def make_table(oracle, tmp_path, rng, n, p=7, counter_size=1, nbins=0, counts=None, k=K, name="db"):
    """sorted unique random k-mers -> a KMC1 (nbins = 0) or KMC2 table; counts default to 0..255 (0 lies outside the header's [1, 255])"""
    km = np.unique(_oracle.random_kmers(rng, n, k).reshape(-1, k), axis=0)
    if counts is None:
        counts = rng.integers(0, 256, size=len(km))
    counts = np.asarray(counts, np.uint32)[: len(km)]
    prefix = str(tmp_path / name)
    flat = np.ascontiguousarray(km).reshape(-1)
    if nbins:
        oracle.kmc2_write(prefix, flat, counts, k, p, counter_size, nbins)
    else:
        oracle.kmc_write(prefix, flat, counts, k, p, counter_size)
    return prefix


def ref_listing(ref, prefix):
    """the reference's CKMCFile::ReadNextKmer over the table (skips counts outside the header's range)"""
    k, mode, cs, p = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    total = ref.l.ref_kmc_total(prefix.encode(), C.byref(k), C.byref(mode), C.byref(cs), C.byref(p))
    assert total >= 0 and k.value == K and mode.value == 0
    km = np.zeros(max(total, 1) * K, np.uint8)
    counts = np.zeros(max(total, 1), np.uint32)
    n = ref.l.ref_kmc_list(prefix.encode(), _ptr(km), _ptr(counts), max(total, 1))
    assert n >= 0
    return km[: n * K], counts[:n]


def gpu_hist(ctx, prefix, ranges=None, count_range=None):
    """bt_kmc_scan_kmer_stats on the device-resident payload, one call per (first, n) range -> (histogram, above-255 count)"""
    from bayestyper_amd import lib

    db = OrcKmc(_oracle.load_oracle(), prefix)
    sc = lib.KmcScan(ctx, db.k, db.p, db.counter_size, db.total, db.lut())
    sc.set_count_range(*(count_range or kmc_count_range(prefix)))
    bins = lib.kmer_stats_bins(db.k)
    d = ctx.to_device(db.payload())
    hist = ctx.buffer(8 * bins).zero()
    over = ctx.buffer(8).zero()
    for first, n in ranges or [(0, db.total)]:
        sc.kmer_stats(d.ptr + first * db.rec_size, first, n, hist.ptr, over.ptr)
    ctx.sync()
    out = hist.download(np.uint64, bins), int(over.download(np.uint64, 1)[0])
    for x in (hist, over, d):
        x.free()
    sc.close()
    db.close()
    return out


def file_hist(ctx, prefix, chunk_records=0, count_range=None):
    from bayestyper_amd import lib

    db = OrcKmc(_oracle.load_oracle(), prefix)
    sc = lib.KmcScan(ctx, db.k, db.p, db.counter_size, db.total, db.lut())
    sc.set_count_range(*(count_range or kmc_count_range(prefix)))
    out = sc.kmer_stats_file(prefix + ".kmc_suf", chunk_records=chunk_records)
    sc.close()
    db.close()
    return out


def parse_output(path, k):
    lines = open(path).read().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    rows = np.array([[int(x) for x in ln.split("\t")] for ln in lines[1:-1]], np.int64).reshape(-1, 6)
    assert np.all(rows[:, 2:].sum(axis=1) == k)
    return rows


def rows_of(hist, k):
    from bayestyper_amd import lib

    return lib.kmer_stats_rows(hist, k)


LAYOUTS = [(3, 0), (7, 0), (11, 0), (7, 1), (7, 3), (7, 4)]   # (p, KMC2 signature bins; 0 = KMC1)


@pytest.mark.parametrize("counter_size", [1, 2, 3, 4])
@pytest.mark.parametrize("p,nbins", LAYOUTS)
def test_parity_with_reference_listing(gpu_ctx, oracle, ref, tmp_path, p, nbins, counter_size):
    """KMC1 at p = 3, 7, 11 and KMC2 with 1, 3, 4 signature bins, counters of 1..4 bytes, counts over 0..255 (and beyond 255 for the wider
    counters: outside the header's [1, 255], so skipped like count 0)"""
    rng = np.random.default_rng(p * 100 + nbins * 10 + counter_size)
    n = 20_000
    counts = rng.integers(0, 256, size=n)
    if counter_size > 1:
        big = rng.random(n) < 0.05
        counts[big] = rng.integers(256, 1 << (8 * min(counter_size, 3)), size=big.sum())
    prefix = make_table(oracle, tmp_path, rng, n, p, counter_size, nbins, counts)
    km, cnt = ref_listing(ref, prefix)
    want, binned, over = expected_hist(km, cnt, K)
    assert over == 0 and 0 < binned < n
    hist, gover = gpu_hist(gpu_ctx, prefix)
    assert gover == 0
    assert np.array_equal(hist, want)


def test_chunking_does_not_matter(gpu_ctx, oracle, ref, tmp_path):
    """several (first, n) ranges — multiples of 16 records, crossing LUT bins of a 4-bin KMC2 table — give the one-call histogram; so does
    the file path with 16-record chunks and with the default chunk"""
    rng = np.random.default_rng(11)
    prefix = make_table(oracle, tmp_path, rng, 60_000, 7, 2, 4)
    db = OrcKmc(oracle, prefix)
    total = db.total
    db.close()
    whole, _ = gpu_hist(gpu_ctx, prefix)
    cuts = np.unique(np.concatenate([[0], rng.integers(1, total // 16, size=9) * 16, [total]]))
    ranges = [(int(a), int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(ranges) >= 5
    split, _ = gpu_hist(gpu_ctx, prefix, ranges)
    assert np.array_equal(split, whole)
    km, cnt = ref_listing(ref, prefix)
    want, binned, _ = expected_hist(km, cnt, K)
    assert np.array_equal(whole, want)
    for chunk in (16, 0):
        hist, nb, over = file_hist(gpu_ctx, prefix, chunk)
        assert np.array_equal(hist, want) and nb == binned and over == 0
    seen = []
    from bayestyper_amd import lib

    db = OrcKmc(oracle, prefix)
    sc = lib.KmcScan(gpu_ctx, db.k, db.p, db.counter_size, db.total, db.lut())
    sc.set_count_range(1, 255)
    hist, _, _ = sc.kmer_stats_file(prefix + ".kmc_suf", chunk_records=4096, progress=seen.append)
    assert np.array_equal(hist, want)
    assert seen == [min(total, 4096 * (i + 1)) for i in range(len(seen))] and seen[-1] == total
    sc.close()
    db.close()


def test_count_range(gpu_ctx, oracle, ref, tmp_path):
    """set_count_range(lo, hi) = the histogram of a table that holds only the in-range records; the executable on a table whose header
    min / max were patched matches the reference's listing of that patched table"""
    rng = np.random.default_rng(5)
    km = np.unique(_oracle.random_kmers(rng, 30_000, K).reshape(-1, K), axis=0)
    counts = rng.integers(1, 256, size=len(km)).astype(np.uint32)
    full = str(tmp_path / "full")
    oracle.kmc_write(full, np.ascontiguousarray(km).reshape(-1), counts, K, 7, 1)
    lo, hi = 3, 200
    keep = (counts >= lo) & (counts <= hi)
    sub = str(tmp_path / "sub")
    oracle.kmc_write(sub, np.ascontiguousarray(km[keep]).reshape(-1), counts[keep], K, 7, 1)
    ranged, _ = gpu_hist(gpu_ctx, full, count_range=(lo, hi))
    only, _ = gpu_hist(gpu_ctx, sub)
    assert np.array_equal(ranged, only)
    assert int(ranged.sum()) == int(keep.sum())
    kmc_patch(full, min_count=lo, max_count=hi)
    rk, rc = ref_listing(ref, full)
    assert len(rc) == keep.sum()
    want, binned, _ = expected_hist(rk, rc, K)
    r = run_exe(full, str(tmp_path / "out"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(parse_output(str(tmp_path / "out_kmer_stats.txt"), K), rows_of(want, K))
    assert f"Wrote statistics for {binned} kmers" in r.stdout


def test_contention_and_edge_compositions(gpu_ctx, oracle, tmp_path):
    """10^6 distinct k-mers with one composition and one count land in one bin exactly (device records and file path); poly-A/C/G/T k-mers
    (a, c, g or t = k) and count 255 on every record"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(1)
    base = np.frombuffer(b"A" * 14 + b"C" * 14 + b"G" * 14 + b"T" * 13, np.uint8)
    km = np.unique(rng.permuted(np.tile(base, (1_000_000, 1)), axis=1), axis=0)
    assert len(km) > 999_000
    prefix = str(tmp_path / "onebin")
    oracle.kmc_write(prefix, np.ascontiguousarray(km).reshape(-1), np.ones(len(km), np.uint32), K, 11, 1)
    ncomp = lib.kmer_stats_bins(K) // 256
    from test_kmer_stats_cpu import comp_index

    want = np.zeros(256 * ncomp, np.uint64)
    want[1 * ncomp + comp_index(K, 14, 14, 14)] = len(km)
    hist, over = gpu_hist(gpu_ctx, prefix)
    assert over == 0 and np.array_equal(hist, want)
    fhist, nb, _ = file_hist(gpu_ctx, prefix)
    assert np.array_equal(fhist, want) and nb == len(km)

    polys = np.array([np.frombuffer(x * K, np.uint8) for x in (b"A", b"C", b"G", b"T")])
    rest = np.unique(_oracle.random_kmers(rng, 5000, K).reshape(-1, K), axis=0)
    km = np.unique(np.concatenate([polys, rest]), axis=0)
    prefix = str(tmp_path / "edges")
    oracle.kmc2_write(prefix, np.ascontiguousarray(km).reshape(-1), np.full(len(km), 255, np.uint32), K, 7, 1, 3)
    want, binned, _ = expected_hist(km.reshape(-1), np.full(len(km), 255), K)
    hist, over = gpu_hist(gpu_ctx, prefix)
    assert over == 0 and np.array_equal(hist, want) and binned == len(km)
    base255 = 255 * ncomp
    for a, c, g in ((K, 0, 0), (0, K, 0), (0, 0, K), (0, 0, 0)):
        assert hist[base255 + comp_index(K, a, c, g)] == 1
    assert hist[:base255].sum() == 0


@pytest.mark.parametrize("k,p", [(31, 7), (63, 7), (64, 8)])
def test_other_kmer_sizes(gpu_ctx, oracle, tmp_path, k, p):
    """k = 31, 63, 64 against the oracle's listing (pinned against the reference at k = 55 in test_oracle_kmer.py); the executable once with
    BT_KMER_SIZE set"""
    rng = np.random.default_rng(k)
    counts = rng.integers(1, 256, size=20_000)
    prefix = make_table(oracle, tmp_path, rng, 20_000, p, 1, 0 if k != 63 else 3, counts, k=k)
    db = OrcKmc(oracle, prefix)
    km, cnt = db.list()
    db.close()
    want, binned, _ = expected_hist(km, cnt, k)
    hist, over = gpu_hist(gpu_ctx, prefix)
    assert over == 0 and np.array_equal(hist, want)
    if k == 31:
        r = run_exe(prefix, str(tmp_path / "out"), k=k)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(parse_output(str(tmp_path / "out_kmer_stats.txt"), k), rows_of(want, k))
        assert f"with a length of {k} nts" in r.stdout and f"Wrote statistics for {binned} kmers" in r.stdout


def test_counts_above_255(gpu_ctx, oracle, tmp_path):
    """the reference asserts count <= 255: such records are counted apart through the ABI and fail the executable, which writes no file"""
    rng = np.random.default_rng(9)
    n = 10_000
    counts = rng.integers(1, 256, size=n)
    big = rng.random(n) < 0.01
    counts[big] = rng.integers(256, 65536, size=big.sum())
    prefix = make_table(oracle, tmp_path, rng, n, 7, 2, 0, counts)
    kmc_patch(prefix, max_count=65535)
    db = OrcKmc(oracle, prefix)
    km, cnt = db.list()
    db.close()
    want, _, nover = expected_hist(km, cnt, K)
    assert nover > 0
    hist, over = gpu_hist(gpu_ctx, prefix)
    assert over == nover and np.array_equal(hist, want)
    fhist, _, fover = file_hist(gpu_ctx, prefix)
    assert fover == nover and np.array_equal(fhist, want)
    r = run_exe(prefix, str(tmp_path / "out"))
    assert r.returncode == 1 and "above 255" in r.stderr and f"{nover} kmer(s)" in r.stderr
    assert not os.path.exists(str(tmp_path / "out_kmer_stats.txt"))


def test_executable_end_to_end(gpu_ctx, oracle, ref, tmp_path):
    """header line, lines = the expected multiset in (count, A, C, G, T) order, the "Wrote statistics for M kmers" line, byte-identical reruns,
    and an empty table (header only)"""
    rng = np.random.default_rng(21)
    prefix = make_table(oracle, tmp_path, rng, 40_000, 7, 1, 4)
    rk, rc = ref_listing(ref, prefix)
    want, binned, _ = expected_hist(rk, rc, K)
    outs = []
    for i in range(2):
        r = run_exe(prefix, str(tmp_path / f"run{i}"))
        assert r.returncode == 0, r.stderr
        assert "Running BayesTyperTools" in r.stdout and "getKmerStats script ..." in r.stdout
        db = OrcKmc(oracle, prefix)
        assert f"Parsing kmer table containing {db.total} unique kmers with a length of {K} nts ..." in r.stdout
        db.close()
        assert f"Wrote statistics for {binned} kmers" in r.stdout and binned == len(rc)
        outs.append(open(str(tmp_path / f"run{i}_kmer_stats.txt"), "rb").read())
    assert outs[0] == outs[1]
    rows = parse_output(str(tmp_path / "run0_kmer_stats.txt"), K)
    assert np.array_equal(rows, rows_of(want, K))
    keys = [tuple(x) for x in rows[:, 1:]]
    assert keys == sorted(keys)
    assert rows[:, 0].sum() == binned

    empty = str(tmp_path / "empty")
    oracle.kmc_write(empty, np.zeros(0, np.uint8), np.zeros(0, np.uint32), K, 7, 1)
    r = run_exe(empty, str(tmp_path / "e"))
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "e_kmer_stats.txt")).read() == HEADER + "\n"
    assert "Wrote statistics for 0 kmers" in r.stdout

