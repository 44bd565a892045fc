"""The executables at a k-mer size other than their default: `bayesTyper cluster` then `genotype` with BT_KMER_SIZE=31 on the C1 dataset
regenerated at k = 31, every file against the oracle pipeline (tests/test_cli_gpu.py's main test at another size: the host graph constructor,
the variant parser, the parameter k-mer order and FASTA, the multigroup order, both stages' filters and tables); and the refusal of inputs
written for another size."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import c1_dataset  # noqa: E402
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu
TOOLS = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")


def test_cluster_then_genotype_at_k31(oracle, tmp_path):
    """two samples (female, male), 300 SNVs on 60 000 nt, all at k = 31.  The parameter k-mer order is that of the reference's HybridHash built
    at k = 31 (oracle/_ref/libbtref_k31.so) when it is present; the multigroup order is the real unordered_set<bitset<62>>'s."""
    CLI.check_cluster_then_genotype(oracle, tmp_path, 60_000, 300, 2, dict(chains=3, burn=12, samples=30), False, None, 0, k=31)


def test_inputs_of_another_kmer_size_are_refused(oracle, tmp_path):
    """BT_KMER_SIZE=31 against the k = 55 dataset: `cluster` refuses the sample Bloom filter, `makeBloom` the KMC database, each with a message
    that names the sizes and exit code 1 — neither computes anything from k-mers of the wrong length"""
    ds = c1_dataset.make(str(tmp_path / "data"), oracle, 20_000, 100, 1, num_error_kmers=5_000)
    env = dict(os.environ, BT_KMER_SIZE="31")
    prefix = str(tmp_path / "bt")
    r = subprocess.run([CLI.EXE, "cluster", "-v", os.path.join(ds["dir"], "candidates.vcf"), "-s", os.path.join(ds["dir"], "samples.tsv"), "-g", os.path.join(ds["dir"], "genome.fa"),
                        "-o", prefix, "-r", "42"], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "Setting the kmer size to 31" in r.stdout, r.stdout[-2000:] + r.stderr
    assert "ERROR: " in r.stderr and "sample1.bloomMeta differs from k" in r.stderr, r.stderr
    assert "completed succesfully" not in r.stdout and not os.path.exists(prefix + "_cluster_data/parameter_kmers.fa.gz")
    kmc = os.path.join(ds["dir"], "sample1")
    before = open(kmc + ".bloomData", "rb").read()
    r = subprocess.run([TOOLS, "makeBloom", "-k", kmc], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and f"ERROR: KMC table {kmc} holds 55-mers, not 31-mers" in r.stderr, r.stdout[-2000:] + r.stderr
    assert open(kmc + ".bloomData", "rb").read() == before
    r = subprocess.run([TOOLS, "makeBloom", "-k", kmc], capture_output=True, text=True)     # and the default size takes it
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
