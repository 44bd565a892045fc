"""A BAM sample through the executables: the C1 plumbing data set of tests/test_reads_cli_gpu.py with sample 2's reads once as FASTQ (the twin) and once as a
BAM.  The BAM holds the twin's reads as mapped, unmapped and reverse-strand records, plus secondary and supplementary copies of some of them that the FASTQ
does not contain: with the default skip flags (0x900) both samples are the same reads, so `makeBloom -r`, `cluster` and `genotype` write the same bytes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bam_data as bd
import c1_dataset
from _oracle import OrcKmc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bayestyper_amd", "bayesTyper")
TOOLS = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
K = 55


def _records(rows, flags):
    """reads of K bases (n, K) uint8 ASCII and their flags -> the records' bytes, laid out once by bam_data.record and filled in with numpy"""
    template = np.frombuffer(bd.record(b"A" * K, name=b"r"), np.uint8)
    seq_at = 36 + 2
    rec = np.tile(template, (len(rows), 1))
    rec[:, 18] = flags & 0xFF
    rec[:, 19] = flags >> 8
    code = np.zeros(256, np.uint8)
    code[[65, 67, 71, 84]] = [1, 2, 4, 8]
    nib = np.zeros((len(rows), K + 1), np.uint8)
    nib[:, :K] = code[rows]
    rec[:, seq_at:seq_at + (K + 1) // 2] = nib[:, 0::2] << 4 | nib[:, 1::2]
    return rec


def _write_sample(oracle, kmc_prefix, d):
    """sample 2's k-mers as reads (each as often as its count says, every other one reverse-complemented) -> r2.reads (a FASTQ) and b2.reads (a BAM)"""
    db = OrcKmc(oracle, kmc_prefix)
    km, counts = db.list()
    total = db.total
    db.close()
    rows = np.repeat(km.reshape(-1, K), counts.astype(np.int64), axis=0)
    comp = np.zeros(256, np.uint8)
    comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    rows[1::2] = comp[rows[1::2, ::-1]]
    fq = np.empty((len(rows), 3 + K + 3 + K + 1), np.uint8)
    fq[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    fq[:, 3:3 + K] = rows
    fq[:, 3 + K:6 + K] = np.frombuffer(b"\n+\n", np.uint8)
    fq[:, 6 + K:6 + 2 * K] = ord("I")
    fq[:, -1] = ord("\n")
    open(os.path.join(d, "r2.fq"), "wb").write(fq.tobytes())
    open(os.path.join(d, "r2.reads"), "w").write("r2.fq\n")
    # the BAM: flags 0 (mapped), 4 (unmapped), 16 (reverse strand) in turn; behind every 50th read a secondary and a supplementary copy of it
    flags = np.array([0, 4, 16], np.uint16)[np.arange(len(rows)) % 3]
    extra = np.arange(0, len(rows), 50)
    order = np.concatenate([np.arange(len(rows)), extra, extra])
    all_flags = np.concatenate([flags, np.full(len(extra), 0x100, np.uint16), np.full(len(extra), 0x800 | 16, np.uint16)])
    o = np.argsort(order, kind="stable")
    body = _records(rows[order[o]], all_flags[o]).tobytes()
    data = bd.header(refs=(("chr1", 100000), ("chr2", 5000))) + body
    stream = bd.bgzf(data, bd.even_cuts(len(data), 65280), level=1)[0]
    open(os.path.join(d, "sample2.sorted.bin"), "wb").write(stream)   # (told by its content, not by its name)
    open(os.path.join(d, "b2.reads"), "w").write("sample2.sorted.bin\n")
    return total, len(rows), len(extra), stream


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam_cli"))
    ds = c1_dataset.make(os.path.join(d, "data"), oracle, 20_000, 100, 2, num_error_kmers=20_000, genders=["F", "M"])
    ds["total2"], ds["reads"], ds["extra"], ds["stream"] = _write_sample(oracle, os.path.join(ds["dir"], "sample2"), ds["dir"])
    for tag, prefix in (("fastq", "r2"), ("bam", "b2")):
        with open(os.path.join(ds["dir"], f"samples_{tag}.tsv"), "w") as f:
            f.write(f"sample1\tF\t{os.path.join(ds['dir'], 'sample1')}\nsample2\tM\t{os.path.join(ds['dir'], prefix)}\n")
    return ds


def _make_bloom(data, prefix, env=None):
    return subprocess.run([TOOLS, "makeBloom", "-r", os.path.join(data["dir"], prefix), "--num-kmers", str(data["total2"]), "-p", "2"], capture_output=True, text=True,
                          env=dict(os.environ, **(env or {})), timeout=120)


def test_make_bloom_from_a_bam_writes_the_twins_bytes(data):
    for prefix in ("r2", "b2"):
        r = _make_bloom(data, prefix)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr
        assert f"Parsed {data['reads'] * K} bases of {data['reads']} reads in 1 file(s)" in r.stdout, r.stdout[-1500:]
    for ext in (".bloomMeta", ".bloomData"):
        assert open(os.path.join(data["dir"], "b2") + ext, "rb").read() == open(os.path.join(data["dir"], "r2") + ext, "rb").read(), ext
    # the estimating pass runs over the device text as well
    est = os.path.join(data["dir"], "est")
    open(est + ".reads", "w").write("sample2.sorted.bin\n")
    r = subprocess.run([TOOLS, "makeBloom", "-r", est], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    m = re.search(r"Estimated (\d+) distinct kmers", r.stdout)
    assert m and abs(int(m.group(1)) - data["total2"]) <= 0.025 * data["total2"], r.stdout[-1500:]   # six standard errors of the sketch (tests/test_reads_cpu.py)


def test_skip_flags_switch_is_honoured(data, tmp_path):
    """BT_BAM_SKIP_FLAGS=0 counts the secondary and supplementary copies too; a value that is no number below 65536 ends the run"""
    prefix = str(tmp_path / "all")
    open(prefix + ".reads", "w").write(os.path.join(data["dir"], "sample2.sorted.bin") + "\n")
    r = subprocess.run([TOOLS, "makeBloom", "-r", prefix, "--num-kmers", str(data["total2"])], capture_output=True, text=True, env=dict(os.environ, BT_BAM_SKIP_FLAGS="0"), timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    n = data["reads"] + 2 * data["extra"]
    assert f"Parsed {n * K} bases of {n} reads" in r.stdout, r.stdout[-1500:]
    r = subprocess.run([TOOLS, "makeBloom", "-r", prefix, "--num-kmers", "1000"], capture_output=True, text=True, env=dict(os.environ, BT_BAM_SKIP_FLAGS="0x100"), timeout=120)
    n = data["reads"] + data["extra"]
    assert r.returncode == 0 and f"Parsed {n * K} bases of {n} reads" in r.stdout, r.stdout[-1500:] + r.stderr
    for bad in ("65536", "secondary", "-1", ""):
        r = subprocess.run([TOOLS, "makeBloom", "-r", prefix, "--num-kmers", "1000"], capture_output=True, text=True, env=dict(os.environ, BT_BAM_SKIP_FLAGS=bad), timeout=120)
        assert r.returncode == 1 and "BT_BAM_SKIP_FLAGS must be a number below 65536" in r.stderr, (bad, r.stderr)


def test_truncated_and_foreign_files_end_the_run(data, tmp_path):
    from bayestyper_amd import lib

    stream = data["stream"]
    second = lib.bgzf_scan_blocks(stream[:200000])[0][1]
    boundary = int(second["in_offset"]) + int(second["in_size"])   # behind the second block: inside a record, and no EOF block follows
    cases = {"cut inside a block": (stream[:len(stream) // 2], "truncated"), "cut at a block boundary": (stream[:boundary], "truncated"),
             "cram": (b"CRAM\x03\x00" + bytes(64), "CRAM is not supported")}
    for name, (content, words) in cases.items():
        prefix = str(tmp_path / name.replace(" ", "_"))
        open(prefix + ".bin", "wb").write(content)
        open(prefix + ".reads", "w").write(os.path.basename(prefix) + ".bin\n")
        r = subprocess.run([TOOLS, "makeBloom", "-r", prefix, "--num-kmers", "1000"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and words in r.stderr, (name, r.stderr[-800:])
        if name == "cut at a block boundary":
            assert "has no BGZF end-of-file block" in r.stderr


def _body(path):
    return [x for x in open(path).read().split("\n") if x and not x.startswith("#")]


def test_genotype_from_a_bam_equals_the_fastq_twin(data, tmp_path):
    """cluster + genotype with samples (KMC, BAM) against (KMC, FASTQ): same seed, same Bloom bytes, so the VCF bodies are equal; the 'Parsed' line reports the
    kept records' bases"""
    for prefix in ("r2", "b2"):
        for ext in (".bloomMeta", ".bloomData"):
            shutil.copy(os.path.join(data["dir"], "sample2") + ext, os.path.join(data["dir"], prefix) + ext)
    common = ["-g", os.path.join(data["dir"], "genome.fa"), "-r", "11"]
    bodies, parsed = [], []
    for tag in ("fastq", "bam"):
        prefix = str(tmp_path / tag)
        sfile = os.path.join(data["dir"], f"samples_{tag}.tsv")
        r = subprocess.run([EXE, "cluster", "-v", os.path.join(data["dir"], "candidates.vcf"), "-s", sfile, "-o", prefix] + common, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr
        r = subprocess.run([EXE, "genotype", "-v", prefix + "_unit_1/variant_clusters.bin", "-c", prefix + "_cluster_data", "-s", sfile, "-o", prefix, "-p", "2",
                            "--number-of-gibbs-chains", "2", "--gibbs-burn-in", "10", "--gibbs-samples", "20"] + common, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        m = re.search(r"Parsed (\d+) bases \((\d+) kmer occurrences passed the path kmer filter\)", r.stdout)
        assert m, r.stdout[-3000:]
        parsed.append((int(m.group(1)), int(m.group(2))))
        bodies.append(_body(prefix + ".vcf"))
    assert parsed[0] == parsed[1] and parsed[0][0] == data["reads"] * K and parsed[0][1] > 0
    assert bodies[0] == bodies[1] and len(bodies[0]) >= 90
    # every record counted: other counts
    prefix = str(tmp_path / "bam")
    sfile = os.path.join(data["dir"], "samples_bam.tsv")
    r = subprocess.run([EXE, "genotype", "-v", prefix + "_unit_1/variant_clusters.bin", "-c", prefix + "_cluster_data", "-s", sfile, "-o", str(tmp_path / "all"), "-p", "2",
                        "--number-of-gibbs-chains", "1", "--gibbs-burn-in", "2", "--gibbs-samples", "2"] + common, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, BT_BAM_SKIP_FLAGS="0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"Parsed (\d+) bases \((\d+) kmer occurrences passed the path kmer filter\)", r.stdout)
    assert m and int(m.group(1)) == (data["reads"] + 2 * data["extra"]) * K and int(m.group(2)) > parsed[1][1], r.stdout[-3000:]
