"""`bayesTyper genotype` with the haplotype candidates kept on the device (the default: bt_paths_candidates_device ->
bt_gibbs_source_create_from_paths, samplers from the unit's source by position) against the same run with BT_CANDIDATES_ON_HOST=1 (the bundle
fetched, assembled on the host and uploaded again): the VCF body, the genomic and the noise parameter files must be identical, whatever the
launch sizing, the mode and the number of ranks.  The default run's stage table must name the device route, so a silent fallback cannot pass."""
import os
import subprocess

import numpy as np
import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
import test_cluster_stage_cpu as T
from _oracle import OrcBloom
from test_cli_gpu import EXE, K, _outputs

pytestmark = pytest.mark.gpu

DEVICE_LABEL = "bt_gibbs_source_create_from_paths"


def _cluster(ds_dir, prefix, seed):
    r = subprocess.run([EXE, "cluster", "-v", os.path.join(ds_dir, "candidates.vcf"), "-s", os.path.join(ds_dir, "samples.tsv"), "-g", os.path.join(ds_dir, "genome.fa"), "-o", prefix,
                        "-r", str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr


def _genotype(prefix, unit_prefix, ds_dir, seed, gibbs, extra_args, env):
    e = dict(os.environ)
    e.pop("BT_CANDIDATES_ON_HOST", None)
    e.update(env)
    e["BT_STAGE_TIMES"] = "1"
    r = subprocess.run([EXE, "genotype", "-v", unit_prefix + "_unit_1/variant_clusters.bin", "-c", unit_prefix + "_cluster_data", "-s", os.path.join(ds_dir, "samples.tsv"), "-g",
                        os.path.join(ds_dir, "genome.fa"), "-o", prefix, "-r", str(seed), "--number-of-gibbs-chains", str(gibbs["chains"]), "--gibbs-burn-in", str(gibbs["burn"]),
                        "--gibbs-samples", str(gibbs["samples"])] + list(extra_args), capture_output=True, text=True, env=e, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "BayesTyper genotype completed succesfully!" in r.stdout
    return r.stdout, r.stderr


def _both_routes(tmp_path, tag, unit_prefix, ds_dir, seed, gibbs, extra_args=(), env=None):
    env = dict(env or {})
    dev, host = str(tmp_path / (tag + "_device")), str(tmp_path / (tag + "_host"))
    out_d, err_d = _genotype(dev, unit_prefix, ds_dir, seed, gibbs, extra_args, env)
    out_h, err_h = _genotype(host, unit_prefix, ds_dir, seed, gibbs, extra_args, dict(env, BT_CANDIDATES_ON_HOST="1"))
    assert DEVICE_LABEL in err_d and "candidates: host arrays + fetch" not in err_d, err_d[-3000:]
    assert DEVICE_LABEL not in err_h and "candidates: host arrays + fetch" in err_h, err_h[-3000:]
    a, b = _outputs(dev), _outputs(host)
    assert a[0] == b[0] and len(a[0]) > 100
    assert a[1] == b[1] and a[2] == b[2]
    return out_d, out_h


@pytest.fixture(scope="module")
def c1(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("c1")
    ds = c1_dataset.make(str(d / "data"), oracle, 70_000, 350, 3, num_error_kmers=150_000, genders=["F", "M", "F"])
    prefix = str(d / "bt")
    _cluster(ds["dir"], prefix, 7)
    return ds["dir"], prefix


GIBBS = dict(chains=3, burn=12, samples=30)


@pytest.mark.parametrize("extra_args,env,launches", [((), {}, None), (("--noise-genotyping",), {}, None), ((), {"BT_MAX_GROUPS_PER_LAUNCH": "23"}, None),
                                                     ((), {"BT_GIBBS_FREE_BYTES": "3000000"}, "launches"),
                                                     ((), {"BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0"}, None),
                                                     (("--noise-genotyping",), {"BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0"}, None)],
                         ids=["default", "noise-genotyping", "23-groups-per-launch", "small-free-bytes", "three-ranks-files", "three-ranks-files-noise-genotyping"])
def test_c1_device_route_equals_host_route(c1, tmp_path, extra_args, env, launches):
    ds_dir, unit_prefix = c1
    out_d, out_h = _both_routes(tmp_path, "run", unit_prefix, ds_dir, 7, GIBBS, extra_args, env)
    if launches:   # the launch sizing (bt_gibbs_state_bytes_from_source on the device route) cut the unit into several launches on both routes, the same way
        cut = [ln.split("] ", 1)[1] for ln in out_d.split("\n") if " launches" in ln and "sampler state" in ln]
        assert cut and cut == [ln.split("] ", 1)[1] for ln in out_h.split("\n") if " launches" in ln and "sampler state" in ln]
    if "BT_GPUS" in env:
        assert "Rank 0 of " in out_d


def test_sv_rich_ten_samples_device_route_equals_host_route(oracle, tmp_path):
    """SNVs, indels, multi-allelic records, MNVs and blocks of structural variants with nested variants (nested variant-cluster groups), ten samples"""
    from test_pipeline_gpu import sample_haplotype

    rng = np.random.default_rng(78)
    seq = "".join(rng.choice(list("ACGT"), 120_000))
    vcf = T.make_vcf(rng, [["chr1", seq, False]], K, 70, False, extra_contig=False, sv_blocks=3)
    records = []
    for line in vcf.split("\n"):
        if line and line[0] != "#":
            _, p, _, r_, alt = line.split("\t")[:5]
            records.append((int(p) - 1, r_, [a for a in alt.split(",") if a != "*"]))
    d = tmp_path / "data"
    os.makedirs(d)
    with open(d / "genome.fa", "w") as fh:
        fh.write(">chr1\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
    open(d / "candidates.vcf", "w").write(vcf)
    with open(d / "samples.tsv", "w") as sf:
        for s, gender in enumerate(["F", "M"] * 5):
            text = "N".join(sample_haplotype(rng, seq, records) for _ in range(2))
            km, va = oracle.kmers_from_sequence(text.encode(), K)
            present = np.unique(km[va == 1], axis=0)
            cnt = (rng.poisson(14, len(present)) + 1).astype(np.uint32)
            asc = oracle.unpack(present, K).reshape(-1, K)
            order = np.lexsort(asc.T[::-1])   # KMC order = ascending ASCII order
            prefix = str(d / f"sample{s + 1}")
            oracle.kmc_write(prefix, np.ascontiguousarray(asc[order]).reshape(-1), cnt[order], K, 7, 1)
            bloom = OrcBloom(oracle, len(present), 1e-3, K)
            bloom.insert(np.ascontiguousarray(asc).reshape(-1))
            bloom.save(prefix)
            bloom.close()
            sf.write(f"sample{s + 1}\t{gender}\t{prefix}\n")
    unit_prefix = str(tmp_path / "bt")
    _cluster(str(d), unit_prefix, 11)
    gibbs = dict(chains=3, burn=10, samples=25)
    _both_routes(tmp_path, "default", unit_prefix, str(d), 11, gibbs)
    _both_routes(tmp_path, "noise", unit_prefix, str(d), 11, gibbs, ("--noise-genotyping",))
