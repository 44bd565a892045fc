"""An ordinary gzip FASTQ sample through the executables: the data set of tests/test_bam_cli_gpu.py with sample 2's reads in two files, one written by
gzip.compress and one sync-flushed every few KB (pigz-like), named by one .reads list.  With BT_FASTQ_GZIP_ON_DEVICE=1 both take the device route
(bt_fastq_gz_scan_text); without it they go through zlib on the host as before.  Same reads, so `makeBloom -r`, `cluster` and `genotype` write the same
bytes either way, and the stage table names the route only with the switch."""
import gzip
import os
import re
import shutil
import subprocess

import pytest

import c1_dataset
import fastq_data as fd
import gunzip_data as gd
from test_bam_cli_gpu import EXE, K, TOOLS, _body, _write_sample

pytestmark = pytest.mark.gpu
ON_DEVICE = {"BT_FASTQ_GZIP_ON_DEVICE": "1", "BT_GUNZIP_CHUNK_BYTES": "4096"}
ROUTE = "gzip FASTQ file(s) on the device"


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gunzip_cli"))
    ds = c1_dataset.make(os.path.join(d, "data"), oracle, 20_000, 100, 2, num_error_kmers=20_000, genders=["F", "M"])
    ds["total2"], ds["reads"], _, _ = _write_sample(oracle, os.path.join(ds["dir"], "sample2"), ds["dir"])
    fastq = open(os.path.join(ds["dir"], "r2.fq"), "rb").read()
    starts = fd.record_starts(fastq)
    half = starts[len(starts) // 2]   # a record boundary
    open(os.path.join(ds["dir"], "g2a.fq.gz"), "wb").write(gzip.compress(fastq[:half]))
    open(os.path.join(ds["dir"], "g2b.fq.gz"), "wb").write(gd.gzip_member(fastq[half:], payload=gd.sync_flushed(fastq[half:], 3)[0]))
    assert gzip.decompress(open(os.path.join(ds["dir"], "g2b.fq.gz"), "rb").read()) == fastq[half:]
    open(os.path.join(ds["dir"], "g2.reads"), "w").write("g2a.fq.gz\ng2b.fq.gz\n")
    with open(os.path.join(ds["dir"], "samples_gzip.tsv"), "w") as f:
        f.write(f"sample1\tF\t{os.path.join(ds['dir'], 'sample1')}\nsample2\tM\t{os.path.join(ds['dir'], 'g2')}\n")
    return ds


def _make_bloom(prefix, num_kmers, env):
    return subprocess.run([TOOLS, "makeBloom", "-r", prefix, "-p", "2", "--num-kmers", str(num_kmers)], capture_output=True, text=True, env=dict(os.environ, BT_STAGE_TIMES="1", **env),
                          timeout=120)


def test_make_bloom_writes_the_same_bytes_with_the_switch(data):
    g2 = os.path.join(data["dir"], "g2")
    parsed = f"Parsed {data['reads'] * K} bases of {data['reads']} reads in 2 file(s)"
    blooms = []
    for env in ({}, ON_DEVICE):
        for ext in (".bloomMeta", ".bloomData"):
            if os.path.exists(g2 + ext):
                os.remove(g2 + ext)
        r = _make_bloom(g2, data["total2"], env)
        assert r.returncode == 0 and parsed in r.stdout, r.stdout[-1500:] + r.stderr
        assert (("(2 " + ROUTE + ")") in r.stderr) == bool(env) and (ROUTE in r.stderr) == bool(env), r.stderr[-1500:]
        blooms.append([open(g2 + ext, "rb").read() for ext in (".bloomMeta", ".bloomData")])
    assert blooms[0] == blooms[1]


def test_genotype_equals_the_run_without_the_switch(data, tmp_path):
    for ext in (".bloomMeta", ".bloomData"):
        shutil.copy(os.path.join(data["dir"], "sample2") + ext, os.path.join(data["dir"], "g2") + ext)
    common = ["-g", os.path.join(data["dir"], "genome.fa"), "-r", "11"]
    sfile = os.path.join(data["dir"], "samples_gzip.tsv")
    bodies, parsed, routes = [], [], []
    for tag, env in (("host", {}), ("device", ON_DEVICE)):
        prefix = str(tmp_path / tag)
        env = dict(os.environ, BT_STAGE_TIMES="1", **env)
        r = subprocess.run([EXE, "cluster", "-v", os.path.join(data["dir"], "candidates.vcf"), "-s", sfile, "-o", prefix] + common, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr
        r = subprocess.run([EXE, "genotype", "-v", prefix + "_unit_1/variant_clusters.bin", "-c", prefix + "_cluster_data", "-s", sfile, "-o", prefix, "-p", "2",
                            "--number-of-gibbs-chains", "2", "--gibbs-burn-in", "10", "--gibbs-samples", "20"] + common, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        m = re.search(r"Parsed (\d+) bases \((\d+) kmer occurrences passed the path kmer filter\)", r.stdout)
        assert m, r.stdout[-3000:]
        parsed.append((int(m.group(1)), int(m.group(2))))
        bodies.append(_body(prefix + ".vcf"))
        routes.append(("(2 " + ROUTE + ")") in r.stderr)
    assert parsed[0] == parsed[1] and parsed[0][0] == data["reads"] * K and parsed[0][1] > 0
    assert bodies[0] == bodies[1] and len(bodies[0]) >= 90
    assert routes == [False, True]


def test_a_damaged_file_ends_the_run(data, tmp_path):
    content = open(os.path.join(data["dir"], "g2a.fq.gz"), "rb").read()
    cases = {"cut": (content[:len(content) // 2], "truncated gzip file"), "crc": (content[:-8] + bytes([content[-8] ^ 1]) + content[-7:], "CRC-32 mismatch (trailer at offset %d)" % (len(content) - 8))}
    for name, (damaged, words) in cases.items():
        prefix = str(tmp_path / name)
        open(prefix + ".fq.gz", "wb").write(damaged)
        open(prefix + ".reads", "w").write(name + ".fq.gz\n")
        r = _make_bloom(prefix, 1000, ON_DEVICE)
        assert r.returncode == 1 and words in r.stderr and "read file " in r.stderr, (name, r.stderr[-800:])
