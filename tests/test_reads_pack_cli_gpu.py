"""The reads pack through the executables: the data set of tests/test_bam_cli_gpu.py with sample 2's reads spread over a plain FASTQ, a .fastq.gz, a BGZF FASTQ
and a BAM in one list.  BT_READS_PACK=1 makes the first pass write <prefix>.reads.pack; later passes stream it and write the bytes of a run from the files."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bam_data as bd
import c1_dataset
from test_bam_cli_gpu import EXE, K, TOOLS, _body, _records, _write_sample

pytestmark = pytest.mark.gpu
FROM_PACK = "(from the reads pack)"
READING = "from the reads pack "
RECORD = 3 + K + 3 + K + 1   # "@r\n" bases "\n+\n" qualities "\n"


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mixed_cli"))
    ds = c1_dataset.make(os.path.join(d, "data"), oracle, 20_000, 100, 2, num_error_kmers=20_000, genders=["F", "M"])
    ds["total2"], ds["reads"], _, _ = _write_sample(oracle, os.path.join(ds["dir"], "sample2"), ds["dir"])
    fastq = open(os.path.join(ds["dir"], "r2.fq"), "rb").read()
    n = len(fastq) // RECORD
    assert n == ds["reads"] and n * RECORD == len(fastq) and n > 2000
    cuts = [0, n // 4, n // 2, 3 * n // 4, n]
    part = [fastq[a * RECORD:b * RECORD] for a, b in zip(cuts, cuts[1:])]
    dd = ds["dir"]
    open(os.path.join(dd, "m_a.fq"), "wb").write(part[0])
    open(os.path.join(dd, "m_b.fastq.gz"), "wb").write(gzip.compress(part[1], 1))
    open(os.path.join(dd, "m_c.fq.gz"), "wb").write(bd.bgzf(part[2], bd.even_cuts(len(part[2]), 65280), level=1)[0])
    rows = np.frombuffer(part[3], np.uint8).reshape(-1, RECORD)[:, 3:3 + K]
    flags = np.array([0, 4, 16], np.uint16)[np.arange(len(rows)) % 3]   # (a reverse-strand record holds the read as it is here: the twin of _write_sample)
    body = bd.header(refs=(("chr1", 100000),)) + _records(rows, flags).tobytes()
    open(os.path.join(dd, "m_d.bam"), "wb").write(bd.bgzf(body, bd.even_cuts(len(body), 65280), level=1)[0])
    ds["list"] = "m_a.fq\nm_b.fastq.gz\nm_c.fq.gz\nm_d.bam\n"
    for prefix in ("m2", "two"):
        open(os.path.join(dd, prefix + ".reads"), "w").write(ds["list"])
    with open(os.path.join(dd, "samples_mixed.tsv"), "w") as f:
        f.write(f"sample1\tF\t{os.path.join(dd, 'sample1')}\nsample2\tM\t{os.path.join(dd, 'm2')}\n")
    return ds


def _make_bloom(prefix, num_kmers, env=None):
    return subprocess.run([TOOLS, "makeBloom", "-r", prefix, "-p", "2"] + (["--num-kmers", str(num_kmers)] if num_kmers else []), capture_output=True, text=True,
                          env=dict({k: v for k, v in os.environ.items() if k != "BT_READS_PACK"}, BT_STAGE_TIMES="1", **(env or {})), timeout=120)


def _bloom_bytes(prefix):
    return [open(prefix + ext, "rb").read() for ext in (".bloomMeta", ".bloomData")]


def _unstamped(text):
    return re.sub(r"\[\d\d/\d\d/\d{4} \d\d:\d\d:\d\d\] ", "", text)


def test_make_bloom_writes_the_pack_and_later_runs_read_it(data):
    from bayestyper_amd import lib

    dd = data["dir"]
    m2 = os.path.join(dd, "m2")
    parsed = f"Parsed {data['reads'] * K} bases of {data['reads']} reads in 4 file(s)"
    # no pack, no variable: the parent's wording, no new file beside the sample
    before = set(os.listdir(dd))
    r = _make_bloom(m2, data["total2"])
    assert r.returncode == 0 and parsed in r.stdout, r.stdout[-1500:] + r.stderr
    assert "reads pack" not in r.stdout and "reads pack" not in r.stderr
    assert set(os.listdir(dd)) - before == {"m2.bloomMeta", "m2.bloomData"}
    assert [x for x in _unstamped(r.stdout).split("\n") if x][-3:] == [parsed, f"Saving bloom filter to {m2} ...", "Completed saving bloom filter"]
    want = _bloom_bytes(m2)
    plain = _unstamped(r.stdout)
    # BT_READS_PACK=1: the same bytes, and the pack beside the list with the totals the run printed
    r = _make_bloom(m2, data["total2"], {"BT_READS_PACK": "1"})
    assert r.returncode == 0 and parsed in r.stdout and f"Wrote the reads pack {m2}.reads.pack" in r.stdout and FROM_PACK not in r.stderr, r.stdout[-1500:] + r.stderr
    assert _bloom_bytes(m2) == want
    assert set(os.listdir(dd)) - before == {"m2.bloomMeta", "m2.bloomData", "m2.reads.pack"}   # no temporary file is left
    info = lib.reads_pack_file_info(m2 + ".reads.pack")
    assert (info["bases"], info["reads"], info["k"]) == (data["reads"] * K, data["reads"], K) and info["sections"] >= 4
    assert info["positions"] == data["reads"] * (K + 1)   # a separator behind every read, whichever reader made the text
    reader = lib.ReadsPackReader(m2 + ".reads.pack")
    manifest = reader.manifest()
    reader.close()
    assert "m_d.bam:" in manifest and f"\nk:{K}\n" in manifest and "\nbam_skip_flags:2304\n" in manifest
    # the pack is there: no variable is needed to read it, with it the run reads it too (and writes none)
    stamp = os.stat(m2 + ".reads.pack").st_mtime_ns
    for env in ({}, {"BT_READS_PACK": "1"}):
        for ext in (".bloomMeta", ".bloomData"):
            os.remove(m2 + ext)
        r = _make_bloom(m2, data["total2"], env)
        assert r.returncode == 0 and parsed in r.stdout and READING + m2 + ".reads.pack" in r.stdout and FROM_PACK in r.stderr, r.stdout[-1500:] + r.stderr
        assert "file(s) on the device)" not in r.stderr and "Wrote the reads pack" not in r.stdout
        assert _bloom_bytes(m2) == want and os.stat(m2 + ".reads.pack").st_mtime_ns == stamp
    # BT_READS_PACK=0 reads the files
    r = _make_bloom(m2, data["total2"], {"BT_READS_PACK": "0"})
    assert r.returncode == 0 and _unstamped(r.stdout) == plain and FROM_PACK not in r.stderr and "BAM file(s) on the device" in r.stderr, r.stdout[-1500:] + r.stderr
    assert _bloom_bytes(m2) == want
    # another value of BT_BAM_SKIP_FLAGS: stale, one warning, the files are read
    r = _make_bloom(m2, data["total2"], {"BT_BAM_SKIP_FLAGS": "0x904"})
    assert r.returncode == 0 and r.stderr.count("is stale") == 1 and "bam_skip_flags:2308" in r.stderr and FROM_PACK not in r.stderr, r.stderr[-1500:]


def test_two_pass_make_bloom_writes_in_the_sketch_pass_and_reads_in_the_filter_pass(data):
    two = os.path.join(data["dir"], "two")
    r = _make_bloom(two, 0)
    assert r.returncode == 0 and "reads pack" not in r.stdout, r.stdout[-1500:] + r.stderr
    want, estimated = _bloom_bytes(two), re.search(r"Estimated (\d+) distinct kmers", r.stdout).group(1)
    r = _make_bloom(two, 0, {"BT_READS_PACK": "1"})
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    out = r.stdout
    assert out.index("Wrote the reads pack") < out.index(f"Estimated {estimated} distinct kmers") < out.index(READING) and out.count("Wrote the reads pack") == 1
    assert FROM_PACK in r.stderr and _bloom_bytes(two) == want
    assert f"Parsed {data['reads'] * K} bases of {data['reads']} reads in 4 file(s)" in out


def _genotype(data, prefix, out, env=None):
    common = ["-g", os.path.join(data["dir"], "genome.fa"), "-r", "11"]
    sfile = os.path.join(data["dir"], "samples_mixed.tsv")
    return subprocess.run([EXE, "genotype", "-v", prefix + "_unit_1/variant_clusters.bin", "-c", prefix + "_cluster_data", "-s", sfile, "-o", out, "-p", "2",
                           "--number-of-gibbs-chains", "1", "--gibbs-burn-in", "5", "--gibbs-samples", "10"] + common, capture_output=True, text=True, timeout=300,
                          env=dict({k: v for k, v in os.environ.items() if k != "BT_READS_PACK"}, BT_STAGE_TIMES="1", **(env or {})))


def test_cluster_and_genotype_from_the_pack_equal_the_run_from_the_files(data, tmp_path):
    """with the pack present `cluster` (which reads the sample's filter, not its reads) and `genotype` give the VCF body of a run that reads the files
    (BT_READS_PACK=0); a stale pack gives one warning and the same body; a damaged section ends the run"""
    dd = data["dir"]
    m2 = os.path.join(dd, "m2")
    pack = m2 + ".reads.pack"
    for ext in (".bloomMeta", ".bloomData"):
        shutil.copy(os.path.join(dd, "sample2") + ext, m2 + ext)
    if not os.path.exists(pack):
        r = _make_bloom(os.path.join(dd, "m2"), data["total2"], {"BT_READS_PACK": "1"})
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr
        for ext in (".bloomMeta", ".bloomData"):
            shutil.copy(os.path.join(dd, "sample2") + ext, m2 + ext)
    prefix = str(tmp_path / "run")
    r = subprocess.run([EXE, "cluster", "-v", os.path.join(dd, "candidates.vcf"), "-s", os.path.join(dd, "samples_mixed.tsv"), "-o", prefix, "-g", os.path.join(dd, "genome.fa"),
                        "-r", "11"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    parsed_re = r"Parsed (\d+) bases \((\d+) kmer occurrences passed the path kmer filter\)"
    r = _genotype(data, prefix, prefix + "_files", {"BT_READS_PACK": "0"})
    assert r.returncode == 0 and "reads pack" not in r.stdout and FROM_PACK not in r.stderr and "BAM file(s) on the device" in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    want, parsed = _body(prefix + "_files.vcf"), re.search(parsed_re, r.stdout).groups()
    assert len(want) >= 90 and int(parsed[0]) == data["reads"] * K and int(parsed[1]) > 0
    r = _genotype(data, prefix, prefix + "_pack")
    assert r.returncode == 0 and READING + pack in r.stdout and "parse sample k-mers (reads route): sample2" in r.stderr and FROM_PACK in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    assert "file(s) on the device)" not in r.stderr
    assert _body(prefix + "_pack.vcf") == want and re.search(parsed_re, r.stdout).groups() == parsed
    # a blank line appended to the list: another size and CRC, so the pack is stale
    with open(m2 + ".reads", "a") as f:
        f.write("\n")
    try:
        r = _genotype(data, prefix, prefix + "_stale")
        assert r.returncode == 0 and r.stderr.count("is stale") == 1 and "list_bytes" in r.stderr and FROM_PACK not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
        assert READING not in r.stdout and _body(prefix + "_stale.vcf") == want and re.search(parsed_re, r.stdout).groups() == parsed
    finally:
        open(m2 + ".reads", "w").write(data["list"])
    # one flipped payload byte in the second section
    from bayestyper_amd import lib

    good = open(pack, "rb").read()
    reader = lib.ReadsPackReader(pack)
    header = 9 + 16 + len(reader.manifest()) + 4
    first = reader.next()
    reader.close()
    second = header + 28 + lib.reads_packed_bytes(first[1]) + 4
    damaged = bytearray(good)
    damaged[second + 28 + 100] ^= 0x40
    open(pack, "wb").write(bytes(damaged))
    try:
        r = _genotype(data, prefix, prefix + "_damaged")
        assert r.returncode != 0 and f"section 1 at offset {second}: CRC mismatch" in r.stderr and pack in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    finally:
        open(pack, "wb").write(good)
