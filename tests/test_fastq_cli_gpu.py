"""A BGZF-compressed FASTQ sample through the executables: the data set of tests/test_bam_cli_gpu.py with sample 2's reads once as a plain FASTQ (r2.fq) and
once as the same bytes compressed as BGZF (z2.fq.gz), which takes the device route (bt_fastq_scan_text).  Same reads, so `makeBloom -r`, `cluster` and
`genotype` write the same bytes; BT_FASTQ_BGZF_ON_HOST=1 sends the compressed file through zlib as before."""
import gzip
import os
import re
import shutil
import subprocess

import pytest

import bam_data as bd
import c1_dataset
import fastq_data as fd
from test_bam_cli_gpu import EXE, K, TOOLS, _body, _write_sample

pytestmark = pytest.mark.gpu
ON_HOST = {"BT_FASTQ_BGZF_ON_HOST": "1"}
ROUTE = "BGZF FASTQ file(s) on the device"


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fastq_cli"))
    ds = c1_dataset.make(os.path.join(d, "data"), oracle, 20_000, 100, 2, num_error_kmers=20_000, genders=["F", "M"])
    ds["total2"], ds["reads"], _, _ = _write_sample(oracle, os.path.join(ds["dir"], "sample2"), ds["dir"])
    ds["fastq"] = open(os.path.join(ds["dir"], "r2.fq"), "rb").read()
    ds["stream"], ds["offsets"] = bd.bgzf(ds["fastq"], bd.even_cuts(len(ds["fastq"]), 65280), level=1)
    open(os.path.join(ds["dir"], "z2.fq.gz"), "wb").write(ds["stream"])
    open(os.path.join(ds["dir"], "z2.reads"), "w").write("z2.fq.gz\n")
    for tag, prefix in (("plain", "r2"), ("bgzf", "z2")):
        with open(os.path.join(ds["dir"], f"samples_{tag}.tsv"), "w") as f:
            f.write(f"sample1\tF\t{os.path.join(ds['dir'], 'sample1')}\nsample2\tM\t{os.path.join(ds['dir'], prefix)}\n")
    return ds


def _make_bloom(prefix, num_kmers, env=None):
    return subprocess.run([TOOLS, "makeBloom", "-r", prefix, "-p", "2"] + (["--num-kmers", str(num_kmers)] if num_kmers else []), capture_output=True, text=True,
                          env=dict(os.environ, **(env or {})), timeout=120)


def _bloom_bytes(prefix):
    return [open(prefix + ext, "rb").read() for ext in (".bloomMeta", ".bloomData")]


def test_make_bloom_from_a_bgzf_fastq_writes_the_twins_bytes(data):
    assert len(data["offsets"]) > 3   # several blocks, so records straddle them (65280 is no multiple of a record's 117 bytes)
    r2, z2 = (os.path.join(data["dir"], p) for p in ("r2", "z2"))
    parsed = f"Parsed {data['reads'] * K} bases of {data['reads']} reads in 1 file(s)"
    r = _make_bloom(r2, data["total2"], {"BT_STAGE_TIMES": "1"})
    assert r.returncode == 0 and parsed in r.stdout and ROUTE not in r.stderr, r.stdout[-1500:] + r.stderr
    want = _bloom_bytes(r2)
    for env, on_device in (({}, True), (ON_HOST, False)):
        for ext in (".bloomMeta", ".bloomData"):
            if os.path.exists(z2 + ext):
                os.remove(z2 + ext)
        r = _make_bloom(z2, data["total2"], dict(env, BT_STAGE_TIMES="1"))
        assert r.returncode == 0 and parsed in r.stdout, r.stdout[-1500:] + r.stderr
        assert (("(1 " + ROUTE + ")") in r.stderr) == on_device, r.stderr[-1500:]
        assert _bloom_bytes(z2) == want, env
    # the estimating pass runs over the device text as well
    est = os.path.join(data["dir"], "est")
    open(est + ".reads", "w").write("z2.fq.gz\n")
    r = _make_bloom(est, 0)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr
    m = re.search(r"Estimated (\d+) distinct kmers", r.stdout)
    assert m and abs(int(m.group(1)) - data["total2"]) <= 0.025 * data["total2"], r.stdout[-1500:]   # six standard errors of the sketch (tests/test_bam_cli_gpu.py)


def test_genotype_from_a_bgzf_fastq_equals_the_plain_twin(data, tmp_path):
    """cluster + genotype with samples (KMC, BGZF FASTQ) against (KMC, plain FASTQ): same seed, same Bloom bytes, so the VCF bodies are equal"""
    for prefix in ("r2", "z2"):
        for ext in (".bloomMeta", ".bloomData"):
            shutil.copy(os.path.join(data["dir"], "sample2") + ext, os.path.join(data["dir"], prefix) + ext)
    common = ["-g", os.path.join(data["dir"], "genome.fa"), "-r", "11"]
    bodies, parsed, routes = [], [], []
    for tag in ("plain", "bgzf"):
        prefix = str(tmp_path / tag)
        sfile = os.path.join(data["dir"], f"samples_{tag}.tsv")
        r = subprocess.run([EXE, "cluster", "-v", os.path.join(data["dir"], "candidates.vcf"), "-s", sfile, "-o", prefix] + common, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr
        r = subprocess.run([EXE, "genotype", "-v", prefix + "_unit_1/variant_clusters.bin", "-c", prefix + "_cluster_data", "-s", sfile, "-o", prefix, "-p", "2",
                            "--number-of-gibbs-chains", "2", "--gibbs-burn-in", "10", "--gibbs-samples", "20"] + common, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, BT_STAGE_TIMES="1"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        m = re.search(r"Parsed (\d+) bases \((\d+) kmer occurrences passed the path kmer filter\)", r.stdout)
        assert m, r.stdout[-3000:]
        parsed.append((int(m.group(1)), int(m.group(2))))
        bodies.append(_body(prefix + ".vcf"))
        routes.append(ROUTE in r.stderr)
    assert parsed[0] == parsed[1] and parsed[0][0] == data["reads"] * K and parsed[0][1] > 0
    assert bodies[0] == bodies[1] and len(bodies[0]) >= 90
    assert routes == [False, True]


def test_damaged_files_end_the_run(data, tmp_path):
    stream, offsets, fastq = data["stream"], data["offsets"], data["fastq"]
    boundary = offsets[2]   # behind the second block: 2 x 65280 bytes of content, which end inside a record; no EOF block follows
    with pytest.raises(fd.FastqError) as at_boundary:
        fd.parse(fastq[:2 * 65280])
    missing = fastq[:117 * 700] + fastq[117 * 700:].replace(b"\n+\n", b"\n", 1)   # record 701 lacks its '+' line
    with pytest.raises(fd.FastqError) as no_plus:
        fd.parse(missing)
    assert str(no_plus.value) == fd.MESSAGES["plus"] % 2803
    head = stream[:offsets[3]]
    cases = {"cut inside a block": (stream[:len(stream) // 2], "the file ends inside the block: truncated"),
             "cut at a block boundary": (stream[:boundary], str(at_boundary.value)),
             "gzip member appended": (head + gzip.compress(fastq[3 * 65280:4 * 65280]), f"BGZF block at offset {len(head)}: not a BGZF block header"),
             "missing line": (bd.bgzf(missing, bd.even_cuts(len(missing), 65280), level=1)[0], str(no_plus.value))}
    for name, (content, words) in cases.items():
        prefix = str(tmp_path / name.replace(" ", "_"))
        open(prefix + ".fq.gz", "wb").write(content)
        open(prefix + ".reads", "w").write(os.path.basename(prefix) + ".fq.gz\n")
        r = _make_bloom(prefix, 1000)
        assert r.returncode == 1 and words in r.stderr, (name, r.stderr[-800:])
        assert ("has no BGZF end-of-file block" in r.stderr) == (name != "missing line"), name
        if name == "gzip member appended":
            assert "BT_FASTQ_BGZF_ON_HOST=1" in r.stderr
        if name == "missing line":   # the host route says the same words about the same file
            h = _make_bloom(prefix, 1000, ON_HOST)
            assert h.returncode == 1, h.stderr[-800:]
            line = [x for x in r.stderr.split("\n") if "read file " in x and ".fq.gz: " in x]
            assert line and line[0].split(".fq.gz: ", 1)[1] == str(no_plus.value)
            assert [x for x in h.stderr.split("\n") if x.endswith(".fq.gz: " + str(no_plus.value))], h.stderr[-800:]
