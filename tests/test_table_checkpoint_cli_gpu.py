"""`bayesTyper genotype` with BT_TABLE_CHECKPOINT=<file>: a run that saves its k-mer table after parseSampleKmers and runs that load it — without the KMC
databases, with another seed, in the other mode, on three ranks — write the files of plain runs, byte for byte; a checkpoint of other inputs or a damaged
one ends the run with exit code 1 and stays as it is."""
import glob
import os
import shutil
import subprocess

import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
from test_candidates_device_cli_gpu import _cluster, _genotype
from test_cli_gpu import EXE, _outputs

pytestmark = pytest.mark.gpu

GIBBS = dict(chains=3, burn=12, samples=30)
LOAD_ROW, SAVE_ROW = "load k-mer table checkpoint", "save k-mer table checkpoint"
SKIPPED_ROWS = ("parameter k-mers", "count path k-mers (enumerate + Bloom insert)", "count inter-cluster k-mers", "parse sample k-mers (KMC scan incl. H2D)")
RANKS = {"BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0"}


def _rows(err):
    """the names of the stage table's rows"""
    table = err.split("## stage times:")[-1].split("\n")[1:]
    return [ln[:52].rstrip() for ln in table if ln.rstrip().endswith(" s")]


@pytest.fixture(scope="module")
def c1(tmp_path_factory, oracle):
    """the data set, its unit, the plain runs (switch unset) of both modes and a checkpoint written by a run of the default mode"""
    d = tmp_path_factory.mktemp("c1")
    ds = c1_dataset.make(str(d / "data"), oracle, 70_000, 350, 3, num_error_kmers=150_000, genders=["F", "M", "F"])
    prefix = str(d / "bt")
    _cluster(ds["dir"], prefix, 7)
    env = {k: v for k, v in os.environ.items()}
    assert "BT_TABLE_CHECKPOINT" not in env
    plain = {}
    for tag, seed, extra in (("default", 7, ()), ("seed11", 11, ()), ("noise", 7, ("--noise-genotyping",))):
        out, err = _genotype(str(d / ("plain_" + tag)), prefix, ds["dir"], seed, GIBBS, extra, {})
        assert "checkpoint" not in out and not any("checkpoint" in r for r in _rows(err)) and all(r in _rows(err) for r in SKIPPED_ROWS)
        plain[tag] = _outputs(str(d / ("plain_" + tag)))
    ckpt = str(d / "table.ckpt")
    out, err = _genotype(str(d / "saving"), prefix, ds["dir"], 7, GIBBS, (), {"BT_TABLE_CHECKPOINT": ckpt})
    assert os.path.exists(ckpt) and not os.path.exists(ckpt + ".tmp") and "Saved the kmer table to checkpoint" in out
    assert SAVE_ROW in _rows(err) and LOAD_ROW not in _rows(err) and all(r in _rows(err) for r in SKIPPED_ROWS)
    assert _outputs(str(d / "saving")) == plain["default"]
    return dict(dir=str(d), ds=ds["dir"], unit=prefix, plain=plain, ckpt=ckpt)


@pytest.fixture()
def without_databases(c1):
    """every .kmc_pre / .kmc_suf / .bloom* of the samples moved away for the duration of a test: whatever runs then has scanned nothing"""
    away = os.path.join(c1["dir"], "away")
    os.makedirs(away)
    moved = [f for pat in ("*.kmc_pre", "*.kmc_suf", "*.bloom*") for f in glob.glob(os.path.join(c1["ds"], pat))]
    assert len(moved) >= 9
    for f in moved:
        shutil.move(f, away)
    yield
    for f in moved:
        shutil.move(os.path.join(away, os.path.basename(f)), f)
    os.rmdir(away)


@pytest.mark.parametrize("tag,seed,extra", [("default", 7, ()), ("seed11", 11, ()), ("noise", 7, ("--noise-genotyping",))], ids=["same-run", "another-seed", "noise-genotyping"])
def test_loading_run_writes_the_plain_runs_files(c1, without_databases, tmp_path, tag, seed, extra):
    import hashlib

    before = hashlib.sha256(open(c1["ckpt"], "rb").read()).hexdigest()
    out, err = _genotype(str(tmp_path / "loading"), c1["unit"], c1["ds"], seed, GIBBS, extra, {"BT_TABLE_CHECKPOINT": c1["ckpt"]})
    rows = _rows(err)
    assert LOAD_ROW in rows and SAVE_ROW not in rows and not [r for r in SKIPPED_ROWS if r in rows], rows
    assert "skipped parsing parameter kmers, the path kmer bloom filter, counting inter-cluster kmers and parsing sample kmers" in out
    assert "Parsing kmers from sample" not in out and "Counting kmers in inter-cluster regions" not in out
    assert _outputs(str(tmp_path / "loading")) == c1["plain"][tag]
    assert hashlib.sha256(open(c1["ckpt"], "rb").read()).hexdigest() == before


def _failing(c1, prefix, env, samples=None):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([EXE, "genotype", "-v", c1["unit"] + "_unit_1/variant_clusters.bin", "-c", c1["unit"] + "_cluster_data", "-s", samples or os.path.join(c1["ds"], "samples.tsv"), "-g",
                        os.path.join(c1["ds"], "genome.fa"), "-o", prefix, "-r", "7", "--number-of-gibbs-chains", "3", "--gibbs-burn-in", "12", "--gibbs-samples", "30"],
                       capture_output=True, text=True, env=e, timeout=600)
    return r


def test_stale_or_damaged_checkpoint_ends_the_run(c1, tmp_path):
    data = open(c1["ckpt"], "rb").read()
    # the samples in another order: sample s owns count byte s, so the table would be another one
    lines = open(os.path.join(c1["ds"], "samples.tsv")).read().strip().split("\n")
    reordered = str(tmp_path / "samples.tsv")
    open(reordered, "w").write("\n".join([lines[1], lines[0], lines[2]]) + "\n")
    r = _failing(c1, str(tmp_path / "stale"), {"BT_TABLE_CHECKPOINT": c1["ckpt"]}, samples=reordered)
    assert r.returncode == 1 and "ERROR: BT_TABLE_CHECKPOINT" in r.stderr and "was written for other inputs" in r.stderr and "manifest line 3 differs" in r.stderr, r.stderr[-2000:]
    assert open(c1["ckpt"], "rb").read() == data and not os.path.exists(str(tmp_path / "stale.vcf"))
    # a flipped byte in the records
    damaged = str(tmp_path / "damaged.ckpt")
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    open(damaged, "wb").write(bytes(flipped))
    r = _failing(c1, str(tmp_path / "damaged"), {"BT_TABLE_CHECKPOINT": damaged})
    assert r.returncode == 1 and "ERROR: BT_TABLE_CHECKPOINT" in r.stderr and "chunk CRC mismatch" in r.stderr, r.stderr[-2000:]
    assert open(damaged, "rb").read() == bytes(flipped) and not os.path.exists(damaged + ".tmp") and not os.path.exists(str(tmp_path / "damaged.vcf"))


def test_three_ranks_save_then_load(c1, tmp_path):
    """the BT_COMM_TRANSPORT=files pattern of test_cli_gpu.py::test_three_ranks_sharing_one_gpu: rank 0 saves the merged table, then every rank loads it"""
    ckpt = str(tmp_path / "ranks.ckpt")
    out, err = _genotype(str(tmp_path / "saving"), c1["unit"], c1["ds"], 7, GIBBS, (), dict(RANKS, BT_TABLE_CHECKPOINT=ckpt))
    assert "Rank 0 of 3" in out and "Merged the sample counts of" in out and SAVE_ROW in _rows(err)
    assert _outputs(str(tmp_path / "saving")) == c1["plain"]["default"]
    # the merged table of three ranks holds the records of a one-rank run's: the two files carry the same set of records
    from bayestyper_amd import lib

    assert lib.table_file_info(ckpt) == lib.table_file_info(c1["ckpt"])
    out, err = _genotype(str(tmp_path / "loading"), c1["unit"], c1["ds"], 7, GIBBS, (), dict(RANKS, BT_TABLE_CHECKPOINT=ckpt))
    assert "Rank 0 of 3" in out and "Merged the sample counts of" not in out and LOAD_ROW in _rows(err) and not [r for r in SKIPPED_ROWS if r in _rows(err)]
    for r_ in (1, 2):
        assert "Loading the kmer table from checkpoint" in open(str(tmp_path / "loading") + f".rank{r_}.log").read()
    assert _outputs(str(tmp_path / "loading")) == c1["plain"]["default"]
