"""`bayesTyper genotype -z` and `bayesTyper cluster` with BT_GZIP_ON_DEVICE=1 (the gz outputs compressed on the device, bt_gzip_save) against the same runs
without the switch: the decompressed files must be identical and the stage table must name the route exactly when the switch is set and applies, so a silent
fallback cannot pass.  Without -z the switch does nothing in `genotype`.  With several ranks, rank 0 writes the file."""
import gzip
import os

import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
from test_candidates_device_cli_gpu import _cluster, _genotype
from test_cli_gpu import _outputs

pytestmark = pytest.mark.gpu

LABEL = "gzip on the device (bt_gzip_save)"
GIBBS = dict(chains=3, burn=12, samples=30)


def _gz_outputs(prefix):
    """_outputs of a -z run: the .vcf.gz decompressed next to it (it must be ONE valid gzip member, the plain file must not exist)"""
    assert not os.path.exists(prefix + ".vcf") and not os.path.exists(prefix + ".vcf.gz.tmp")
    with open(prefix + ".vcf", "wb") as f:
        f.write(gzip.open(prefix + ".vcf.gz").read())
    out = _outputs(prefix)
    os.remove(prefix + ".vcf")
    return out


@pytest.fixture(scope="module")
def c1(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("c1")
    ds = c1_dataset.make(str(d / "data"), oracle, 70_000, 350, 3, num_error_kmers=150_000, genders=["F", "M", "F"])
    prefix = str(d / "bt")
    _cluster(ds["dir"], prefix, 7)
    base = str(d / "base")   # the parent's route: -z, no switch
    out, err = _genotype(base, prefix, ds["dir"], 7, GIBBS, ("-z",), {})
    assert LABEL not in err and "write VCF (sort + output)" in err
    return ds["dir"], prefix, _gz_outputs(base)


def test_genotype_z_on_the_device(c1, tmp_path):
    ds_dir, unit_prefix, base = c1
    on = str(tmp_path / "on")
    out, err = _genotype(on, unit_prefix, ds_dir, 7, GIBBS, ("-z",), {"BT_GZIP_ON_DEVICE": "1"})
    assert "write VCF (sort + output), " + LABEL in err, err[-3000:]
    got = _gz_outputs(on)
    assert got[0] == base[0] and len(got[0]) > 100 and got[1] == base[1] and got[2] == base[2]
    # a switch value other than 1 is the parent's route
    off = str(tmp_path / "off")
    out, err = _genotype(off, unit_prefix, ds_dir, 7, GIBBS, ("-z",), {"BT_GZIP_ON_DEVICE": "0"})
    assert LABEL not in err and _gz_outputs(off)[0] == base[0]


def test_switch_without_z_does_nothing(c1, tmp_path):
    ds_dir, unit_prefix, base = c1
    plain = str(tmp_path / "plain")
    out, err = _genotype(plain, unit_prefix, ds_dir, 7, GIBBS, (), {"BT_GZIP_ON_DEVICE": "1"})
    assert LABEL not in err and not os.path.exists(plain + ".vcf.gz")
    got = _outputs(plain)
    assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2]


def test_cluster_on_the_device_feeds_genotype(c1, tmp_path, monkeypatch):
    import subprocess

    from test_candidates_device_cli_gpu import EXE

    ds_dir, unit_prefix, base = c1
    prefix = str(tmp_path / "bt")
    env = dict(os.environ, BT_GZIP_ON_DEVICE="1", BT_STAGE_TIMES="1")
    r = subprocess.run([EXE, "cluster", "-v", os.path.join(ds_dir, "candidates.vcf"), "-s", os.path.join(ds_dir, "samples.tsv"), "-g", os.path.join(ds_dir, "genome.fa"), "-o", prefix,
                        "-r", "7"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "inter-cluster regions: " + LABEL in r.stderr and "parameter k-mers: " + LABEL in r.stderr, r.stderr[-3000:]
    for name in ("parameter_kmers.fa.gz", "intercluster_regions.txt.gz"):   # the same content as the parent-route cluster files
        mine, theirs = gzip.open(os.path.join(prefix + "_cluster_data", name)).read(), gzip.open(os.path.join(unit_prefix + "_cluster_data", name)).read()
        assert mine == theirs and len(mine) > 0
    run = str(tmp_path / "run")
    _genotype(run, prefix, ds_dir, 7, GIBBS, ("-z",), {})
    got = _gz_outputs(run)
    assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2]


def test_three_ranks_rank0_writes_the_file(c1, tmp_path):
    ds_dir, unit_prefix, base = c1
    many = str(tmp_path / "many")
    out, err = _genotype(many, unit_prefix, ds_dir, 7, GIBBS, ("-z",), {"BT_GZIP_ON_DEVICE": "1", "BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0"})
    assert "Rank 0 of " in out and "write VCF (sort + output), " + LABEL in err, err[-3000:]
    got = _gz_outputs(many)
    assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2]
