"""CPU tests of the `getKmerStats` executable (src/bayesTyperTools/scripts/getKmerStats.cpp): usage and every error that needs no GPU — the
executable is only run up to the point where it would create a GPU context.  Also the helpers the GPU tests share: the expected histogram
from a k-mer listing, and patching a KMC table's header (mode, min / max count) as bayestyper_amd/host/KmcFile.cpp reads it."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _oracle  # noqa: E402

EXE = os.path.join(ROOT, "bayestyper_amd", "getKmerStats")
USAGE = "USAGE: getKmerStats <kmc_table_prefix> <output_prefix>"
HEADER = "NumberOfKmers\tKmerCount\tAdenineCount\tCytosineCount\tGuanineCount\tThymineCount"


def run_exe(*args, k=None):
    env = dict(os.environ)
    if k is not None:
        env["BT_KMER_SIZE"] = str(k)
    return subprocess.run([EXE, *args], capture_output=True, text=True, env=env)


def comp_index(k, a, c, g):
    """the bin of a composition inside one count (include/btgpu.h: bt_kmer_stats_num_bins)"""
    tri = lambda m: (m + 1) * (m + 2) // 2              # noqa: E731
    tet = lambda m: (m + 1) * (m + 2) * (m + 3) // 6    # noqa: E731
    return tet(k) - tet(k - a) + tri(k - a) - tri(k - a - c) + g


def expected_hist(kmers_ascii, counts, k):
    """getKmerStats.cpp's loop over a listing (ReadNextKmer order): count each k-mer's letters, one bin per (count, A, C, G, T).
    Returns (histogram, number of k-mers binned, number above 255)."""
    km = np.asarray(kmers_ascii, np.uint8).reshape(-1, k)
    counts = np.asarray(counts, np.int64)
    a, c, g = ((km == ord(x)).sum(axis=1).astype(np.int64) for x in "ACG")
    assert np.all(a + c + g + (km == ord("T")).sum(axis=1) == k)
    ok = counts <= 255
    ncomp = (k + 1) * (k + 2) * (k + 3) // 6
    bins = counts[ok] * ncomp + comp_index(k, a[ok], c[ok], g[ok])
    return np.bincount(bins, minlength=256 * ncomp).astype(np.uint64), int(ok.sum()), int((~ok).sum())


def kmc_header_fields(prefix):
    """byte offsets of (mode, min_count, max_count) in <prefix>.kmc_pre: KMC1 header words 0 (mode << 32) and 2 (min | max << 32), KMC2 ("0x200")
    header fields 1, 5 and 6 (KmcFile.cpp, kmc_file.cpp:186-292)"""
    data = open(prefix + ".kmc_pre", "rb").read()
    size = len(data)
    version, = struct.unpack_from("<I", data, size - 12)
    h = size - 8 - data[size - 8]
    return (h + 4, h + 20, h + 24) if version == 0x200 else (h + 4, h + 16, h + 20)


def kmc_count_range(prefix):
    data = open(prefix + ".kmc_pre", "rb").read()
    _, lo, hi = kmc_header_fields(prefix)
    return struct.unpack_from("<I", data, lo)[0], struct.unpack_from("<I", data, hi)[0]


def kmc_patch(prefix, mode=None, min_count=None, max_count=None):
    data = bytearray(open(prefix + ".kmc_pre", "rb").read())
    for at, value in zip(kmc_header_fields(prefix), (mode, min_count, max_count)):
        if value is not None:
            struct.pack_into("<I", data, at, value)
    open(prefix + ".kmc_pre", "wb").write(bytes(data))


def small_table(oracle, tmp_path, k=55, p=7, n=500, name="db", kmc2=False):
    rng = np.random.default_rng(k * 1000 + n)
    km = np.unique(_oracle.random_kmers(rng, n, k).reshape(-1, k), axis=0)
    counts = rng.integers(1, 256, size=len(km)).astype(np.uint32)
    prefix = str(tmp_path / name)
    if kmc2:
        oracle.kmc2_write(prefix, np.ascontiguousarray(km).reshape(-1), counts, k, p, 1, 3)
    else:
        oracle.kmc_write(prefix, np.ascontiguousarray(km).reshape(-1), counts, k, p, 1)
    return prefix, np.ascontiguousarray(km).reshape(-1), counts


def test_usage_for_wrong_argument_counts(tmp_path):
    for args in ((), ("a",), ("a", "b", "c")):
        r = run_exe(*args)
        assert r.returncode == 1 and USAGE in r.stdout, (args, r.stdout, r.stderr)
    assert not os.listdir(tmp_path)


def test_missing_table(tmp_path):
    prefix = str(tmp_path / "nothere")
    r = run_exe(prefix, str(tmp_path / "out"))
    assert r.returncode == 1 and f"ERROR: Unable to open KMC table {prefix}" in r.stderr
    assert "Running BayesTyperTools" in r.stdout and "getKmerStats script" in r.stdout
    assert not os.path.exists(str(tmp_path / "out_kmer_stats.txt"))


def test_kmer_size_mismatch(oracle, tmp_path):
    prefix, _, _ = small_table(oracle, tmp_path, k=31, p=3)
    r = run_exe(prefix, str(tmp_path / "out"))   # BT_KMER_SIZE defaults to 55
    assert r.returncode == 1 and "holds 31-mers, not 55-mers" in r.stderr
    assert not os.path.exists(str(tmp_path / "out_kmer_stats.txt"))


@pytest.mark.parametrize("kmc2", [False, True])
def test_mode_1_table_is_refused(oracle, tmp_path, kmc2):
    prefix, _, _ = small_table(oracle, tmp_path, kmc2=kmc2)
    kmc_patch(prefix, mode=1)
    r = run_exe(prefix, str(tmp_path / "out"))
    assert r.returncode == 1 and "mode 1" in r.stderr and "ERROR:" in r.stderr
    assert not os.path.exists(str(tmp_path / "out_kmer_stats.txt"))


def test_output_directory_missing(oracle, tmp_path):
    prefix, _, _ = small_table(oracle, tmp_path)
    out = str(tmp_path / "no" / "such" / "dir" / "out")
    r = run_exe(prefix, out)
    assert r.returncode == 1 and f"ERROR: Unable to write file {out}_kmer_stats.txt" in r.stderr
    assert "Parsing kmer table" not in r.stdout   # checked before the scan


def test_header_patch_round_trip(oracle, tmp_path):
    """the test helper writes the fields KmcFile reads: the KMC1 and KMC2 writers both store [1, 255]"""
    for kmc2 in (False, True):
        prefix, _, _ = small_table(oracle, tmp_path, name=f"t{int(kmc2)}", kmc2=kmc2)
        assert kmc_count_range(prefix) == (1, 255)
        kmc_patch(prefix, min_count=3, max_count=65535)
        assert kmc_count_range(prefix) == (3, 65535)


def test_expected_histogram_helper():
    """bins enumerate the compositions in (A, C, G) order inside each count; T = k - A - C - G"""
    k = 4
    km = np.frombuffer(b"AAAA" + b"TTTT" + b"ACGT" + b"ACGT" + b"CCCC", np.uint8)
    hist, binned, over = expected_hist(km, [1, 255, 7, 7, 300], k)
    ncomp = 35
    assert len(hist) == 256 * ncomp and binned == 4 and over == 1 and hist.sum() == 4
    assert hist[1 * ncomp + comp_index(k, 4, 0, 0)] == 1
    assert hist[255 * ncomp + 0] == 1   # TTTT: A = C = G = 0
    assert hist[7 * ncomp + comp_index(k, 1, 1, 1)] == 2
    order = [(a, c, g) for a in range(k + 1) for c in range(k + 1 - a) for g in range(k + 1 - a - c)]
    assert [comp_index(k, *x) for x in order] == list(range(ncomp))


def test_fails_loudly_without_gpu(oracle, tmp_path):
    from bayestyper_amd import lib

    n = C.c_int(-1)
    assert lib.bt_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("a GPU is present")
    prefix, _, _ = small_table(oracle, tmp_path)
    r = run_exe(prefix, str(tmp_path / "out"))
    assert r.returncode != 0 and "no HIP device" in r.stderr
    assert "Parsing kmer table containing" in r.stdout
    assert not os.path.exists(str(tmp_path / "out_kmer_stats.txt"))
