"""`bayesTyper genotype` with the genotype summaries computed on the device (BT_GENOTYPES_ON_HOST=0: bt_gibbs_genotypes per launch, one string of
records copied to the host — or gathered to rank 0 — and formatted) against the same run with BT_GENOTYPES_ON_HOST=1 (the collected samples fetched
and summarised by getGenotypes on the host threads): the VCF body, the genomic and the noise parameter files must be identical, whatever the launch
sizing, the mode and the number of ranks.  Each run's stage table must name the route asked for, so a silent fallback cannot pass."""
import os

import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
from test_candidates_device_cli_gpu import _cluster, _genotype
from test_cli_gpu import _outputs

pytestmark = pytest.mark.gpu

DEVICE_LABEL = "bt_gibbs_genotypes"
HOST_LABEL = "genotypes (getGenotypes + VCF lines, -p host threads)"
HOST_FETCH_LABELS = ("Gibbs: result fetch", "Gibbs: result string", "gather of the collected samples")


def _both_routes(tmp_path, tag, unit_prefix, ds_dir, seed, gibbs, extra_args=(), env=None):
    env = dict(env or {})
    dev, host = str(tmp_path / (tag + "_device")), str(tmp_path / (tag + "_host"))
    out_d, err_d = _genotype(dev, unit_prefix, ds_dir, seed, gibbs, extra_args, dict(env, BT_GENOTYPES_ON_HOST="0"))
    out_h, err_h = _genotype(host, unit_prefix, ds_dir, seed, gibbs, extra_args, dict(env, BT_GENOTYPES_ON_HOST="1"))
    assert DEVICE_LABEL in err_d and HOST_LABEL not in err_d and not any(x in err_d for x in HOST_FETCH_LABELS), err_d[-3000:]
    assert DEVICE_LABEL not in err_h and HOST_LABEL in err_h, err_h[-3000:]
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
    if launches:   # the unit was cut into several launches on both routes, the same way: several strings of records on the device route
        cut = [ln.split("] ", 1)[1] for ln in out_d.split("\n") if " launches" in ln and "sampler state" in ln]
        assert cut and cut == [ln.split("] ", 1)[1] for ln in out_h.split("\n") if " launches" in ln and "sampler state" in ln]
    if "BT_GPUS" in env:
        assert "Rank 0 of " in out_d and "bytes of genotype strings (bt_gibbs_genotypes) on this rank" in out_d and "genotype strings" not in out_h


def test_gather_from_host_implies_the_host_route(c1, tmp_path):
    ds_dir, unit_prefix = c1
    env = {"BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0", "BT_GATHER_FROM_HOST": "1", "BT_GENOTYPES_ON_HOST": "0"}
    _, err = _genotype(str(tmp_path / "run"), unit_prefix, ds_dir, 7, GIBBS, (), env)
    assert DEVICE_LABEL not in err and HOST_LABEL in err


def test_sv_rich_ten_samples_device_route_equals_host_route(oracle, tmp_path):
    """SNVs, indels, multi-allelic records, MNVs and blocks of structural variants with nested variants (nested variant-cluster groups), ten samples"""
    import numpy as np

    import test_cluster_stage_cpu as T
    from _oracle import OrcBloom
    from test_cli_gpu import K
    from test_pipeline_gpu import sample_haplotype

    rng = np.random.default_rng(78)
    seq = "".join(rng.choice(list("ACGT"), 120_000))
    vcf = T.make_vcf(rng, [["chr1", seq, False]], K, 70, False, extra_contig=False, sv_blocks=3)
    records = []
    for line in vcf.split("\n"):
        if line and line[0] != "#":
            _, p, _, r_, alt = line.split("\t")[:5]
            records.append((int(p) - 1, r_, [a for a in alt.split(",") if a != "*"]))
    assert any(len(r[2]) > 1 for r in records), "the unit should hold multi-allelic records"
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
