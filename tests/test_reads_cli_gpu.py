"""The reads route through the executables: a sample with a `<prefix>.reads` list and no KMC database goes through `bayesTyperTools makeBloom -r`,
`bayesTyper cluster` and `bayesTyper genotype` to what its KMC twin gives.  The data set is tests/c1_dataset.py's, at a small setting; the reads are the
database's k-mers, each written as many times as its count says (every other one as its reverse complement), as FASTQ: the database is then exactly what KMC
would count from them with canonical counting, -ci1 and the default -cs255."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import c1_dataset
from _oracle import OrcKmc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bayestyper_amd", "bayesTyper")
TOOLS = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
K = 55
SKETCH_BOUND = 0.025   # six standard errors of a 2^16-register sketch (tests/test_reads_cpu.py)


def _write_reads(oracle, kmc_prefix, reads_prefix):
    """the k-mers of a KMC database as reads -> <reads_prefix>.reads naming a gzipped and a plain FASTQ file; returns the database's k-mer count"""
    db = OrcKmc(oracle, kmc_prefix)
    km, counts = db.list()
    total = db.total
    db.close()
    rows = np.repeat(km.reshape(-1, K), counts.astype(np.int64), axis=0)
    comp = np.zeros(256, np.uint8)
    comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    rows[1::2] = comp[rows[1::2, ::-1]]
    rec = np.empty((len(rows), 3 + K + 3 + K + 1), np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    rec[:, 3:3 + K] = rows
    rec[:, 3 + K:6 + K] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + K:6 + 2 * K] = ord("I")
    rec[:, -1] = ord("\n")
    half = len(rec) // 2
    d, base = os.path.dirname(reads_prefix), os.path.basename(reads_prefix)
    with open(os.path.join(d, base + "_1.fq.gz"), "wb") as f:
        f.write(gzip.compress(rec[:half].tobytes(), compresslevel=1))
    with open(os.path.join(d, base + "_2.fq"), "wb") as f:
        f.write(rec[half:].tobytes())
    with open(reads_prefix + ".reads", "w") as f:
        f.write(f"{base}_1.fq.gz\n{os.path.join(d, base)}_2.fq\n")   # a relative and an absolute path
    return total


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reads_cli"))
    ds = c1_dataset.make(os.path.join(d, "data"), oracle, 20_000, 100, 2, num_error_kmers=20_000, genders=["F", "M"])
    ds["reads2"] = os.path.join(ds["dir"], "r2")   # sample 2 again, as reads
    ds["total2"] = _write_reads(oracle, os.path.join(ds["dir"], "sample2"), ds["reads2"])
    with open(os.path.join(ds["dir"], "samples_mixed.tsv"), "w") as f:
        f.write(f"sample1\tF\t{os.path.join(ds['dir'], 'sample1')}\nsample2\tM\t{ds['reads2']}\n")
    return ds


def test_make_bloom_from_reads(data, tmp_path):
    """`makeBloom -r --num-kmers <the database's k-mer count>` writes the bytes `makeBloom -k` writes; without --num-kmers the estimate it prints and sizes the
    filter with is within the sketch's bound"""
    kmc = str(tmp_path / "kmc")
    for ext in (".kmc_pre", ".kmc_suf"):
        shutil.copy(os.path.join(data["dir"], "sample2") + ext, kmc + ext)
    r = subprocess.run([TOOLS, "makeBloom", "-k", kmc], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    r = subprocess.run([TOOLS, "makeBloom", "-r", data["reads2"], "--num-kmers", str(data["total2"]), "-p", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    assert f"Using the given number of {data['total2']} distinct kmers" in r.stdout and "Completed saving bloom filter" in r.stdout
    for ext in (".bloomMeta", ".bloomData"):
        assert open(data["reads2"] + ext, "rb").read() == open(kmc + ext, "rb").read(), ext
    # the estimating pass (the list is copied: the files above stay for the genotype test)
    est_prefix = str(tmp_path / "est")
    open(est_prefix + ".reads", "w").write("".join(os.path.join(data["dir"], os.path.basename(data["reads2"])) + s + "\n" for s in ("_1.fq.gz", "_2.fq")))
    r = subprocess.run([TOOLS, "makeBloom", "-r", est_prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    m = re.search(r"Estimated (\d+) distinct kmers", r.stdout)
    assert m, r.stdout[-1500:]
    print(f"k-mers {data['total2']}, estimate {m.group(1)}")
    assert abs(int(m.group(1)) - data["total2"]) <= SKETCH_BOUND * data["total2"]
    assert open(est_prefix + ".bloomMeta").read().split("\t")[0].strip() != ""
    # exactly one of -k and -r
    r = subprocess.run([TOOLS, "makeBloom", "-k", kmc, "-r", data["reads2"]], capture_output=True, text=True)
    assert r.returncode == 1 and "exactly one of the options" in r.stderr
    r = subprocess.run([TOOLS, "makeBloom", "-p", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "exactly one of the options" in r.stderr


def _body(path):
    return [x for x in open(path).read().split("\n") if x and not x.startswith("#")]


def test_genotype_from_reads_equals_the_kmc_route(data, tmp_path):
    """cluster + genotype with samples (KMC, reads) against (KMC, KMC): the Bloom files are copies, the seed is the same, so the VCF bodies are equal"""
    for ext in (".bloomMeta", ".bloomData"):
        shutil.copy(os.path.join(data["dir"], "sample2") + ext, data["reads2"] + ext)
    common = ["-g", os.path.join(data["dir"], "genome.fa"), "-r", "11"]
    bodies = []
    for tag, samples in (("kmc", "samples.tsv"), ("mixed", "samples_mixed.tsv")):
        prefix = str(tmp_path / tag)
        sfile = os.path.join(data["dir"], samples)
        r = subprocess.run([EXE, "cluster", "-v", os.path.join(data["dir"], "candidates.vcf"), "-s", sfile, "-o", prefix] + common, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr
        r = subprocess.run([EXE, "genotype", "-v", prefix + "_unit_1/variant_clusters.bin", "-c", prefix + "_cluster_data", "-s", sfile, "-o", prefix, "-p", "2",
                            "--number-of-gibbs-chains", "2", "--gibbs-burn-in", "10", "--gibbs-samples", "20"] + common, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        if tag == "mixed":
            m = re.search(r"Parsed (\d+) bases \((\d+) kmer occurrences passed the path kmer filter\)", r.stdout)
            assert m and int(m.group(1)) % K == 0 and int(m.group(2)) > 0, r.stdout[-3000:]
            assert len(re.findall(r"Parsed \d+ kmers \(\d+ passed the path kmer filter\)", r.stdout)) == 1   # sample 1, from its database
        bodies.append(_body(prefix + ".vcf"))
    assert bodies[0] == bodies[1] and len(bodies[0]) >= 90


def test_several_ranks_refuse_a_reads_sample(data, tmp_path):
    """BT_GPUS=2 with a reads sample ends with one message before a rank is started or a device opened"""
    env = dict(os.environ, BT_GPUS="2", BT_DEVICE="7")   # (a device this run never gets to open)
    r = subprocess.run([EXE, "genotype", "-v", str(tmp_path / "no_unit.bin"), "-c", str(tmp_path), "-s", os.path.join(data["dir"], "samples_mixed.tsv"), "-g",
                        os.path.join(data["dir"], "genome.fa"), "-o", str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1
    assert "sample sample2 has a reads list and no KMC database: the reads route runs on one GPU only" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if ".rank" in f or "comm_id" in f]


def test_table_checkpoint_lists_the_read_files(data, tmp_path):
    """BT_TABLE_CHECKPOINT with a reads sample: the manifest's line of the sample lists the .reads file and every read file; a second run loads the table and
    writes the same VCF; a changed read file is another manifest"""
    from bayestyper_amd import lib

    for ext in (".bloomMeta", ".bloomData"):
        shutil.copy(os.path.join(data["dir"], "sample2") + ext, data["reads2"] + ext)
    sfile = os.path.join(data["dir"], "samples_mixed.tsv")
    common = ["-s", sfile, "-g", os.path.join(data["dir"], "genome.fa"), "-r", "11"]
    unit = str(tmp_path / "u")
    r = subprocess.run([EXE, "cluster", "-v", os.path.join(data["dir"], "candidates.vcf"), "-o", unit] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    ckpt = str(tmp_path / "table.ckpt")
    env = dict(os.environ, BT_TABLE_CHECKPOINT=ckpt)
    bodies = []
    for tag in ("save", "load"):
        prefix = str(tmp_path / tag)
        r = subprocess.run([EXE, "genotype", "-v", unit + "_unit_1/variant_clusters.bin", "-c", unit + "_cluster_data", "-o", prefix, "--number-of-gibbs-chains", "2",
                            "--gibbs-burn-in", "10", "--gibbs-samples", "20"] + common, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert ("Saved the kmer table to checkpoint" if tag == "save" else "Loaded ") in r.stdout
        assert ("kmer occurrences passed the path kmer filter" in r.stdout) == (tag == "save")
        bodies.append(_body(prefix + ".vcf"))
    assert bodies[0] == bodies[1] and len(bodies[0]) >= 90
    line = [x for x in lib.table_file_info(ckpt)["manifest"].split("\n") if x.startswith("sample.1.kmc=")]
    assert len(line) == 1 and line[0].startswith("sample.1.kmc=reads list_bytes:") and " files:2 " in line[0]
    for name in ("r2_1.fq.gz", "r2_2.fq"):
        assert f" {name}:{os.path.getsize(os.path.join(data['dir'], name))}" in line[0]
    # the list names another file: the checkpoint is not this run's
    other = os.path.join(data["dir"], "r3")
    shutil.copy(os.path.join(data["dir"], "r2_2.fq"), other + "_2.fq")
    open(other + ".reads", "w").write("r2_1.fq.gz\nr3_2.fq\n")
    for ext in (".bloomMeta", ".bloomData"):
        shutil.copy(data["reads2"] + ext, other + ext)
    sfile3 = str(tmp_path / "samples3.tsv")
    open(sfile3, "w").write(open(sfile).read().replace(data["reads2"], other))
    r = subprocess.run([EXE, "genotype", "-v", unit + "_unit_1/variant_clusters.bin", "-c", unit + "_cluster_data", "-o", str(tmp_path / "other"), "-s", sfile3, "-g",
                        os.path.join(data["dir"], "genome.fa"), "-r", "11"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 1 and "BT_TABLE_CHECKPOINT" in r.stderr
