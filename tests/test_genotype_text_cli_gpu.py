"""`bayesTyper genotype` with BT_GENOTYPE_TEXT_ON_DEVICE=1 (the genotype-derived text of every VCF line formatted on the device, bt_gibbs_genotype_text) against
the same run without the switch: the VCF body, the genomic and the noise parameter files must be identical, whatever the launch sizing and the mode.  The stage
table must name the route, so a silent fallback cannot pass; with several ranks the switch is reported as ignored."""
import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
from test_candidates_device_cli_gpu import _cluster, _genotype
from test_cli_gpu import _outputs

pytestmark = pytest.mark.gpu

TEXT_LABELS = ("genotype text on the device (bt_gibbs_genotype_text + copies)", "VCF lines from the device's text (-p host threads)")
RECORDS_LABEL = "VCF lines from the records of bt_gibbs_genotypes"
IGNORED = "BT_GENOTYPE_TEXT_ON_DEVICE is ignored in a run of several ranks"


def _with_and_without(tmp_path, tag, unit_prefix, ds_dir, seed, gibbs, extra_args=(), env=None, ranks=False):
    env = dict(env or {})
    on, off = str(tmp_path / (tag + "_text")), str(tmp_path / (tag + "_records"))
    out_t, err_t = _genotype(on, unit_prefix, ds_dir, seed, gibbs, extra_args, dict(env, BT_GENOTYPE_TEXT_ON_DEVICE="1"))
    out_r, err_r = _genotype(off, unit_prefix, ds_dir, seed, gibbs, extra_args, env)
    if ranks:
        assert out_t.count(IGNORED) == 1 and not any(x in err_t for x in TEXT_LABELS) and RECORDS_LABEL in err_t, (out_t[-2000:], err_t[-3000:])
    else:
        assert all(x in err_t for x in TEXT_LABELS) and RECORDS_LABEL not in err_t and "records route" not in err_t and IGNORED not in out_t, err_t[-3000:]
    assert not any(x in err_r for x in TEXT_LABELS) and RECORDS_LABEL in err_r and IGNORED not in out_r, err_r[-3000:]
    a, b = _outputs(on), _outputs(off)
    assert a[0] == b[0] and len(a[0]) > 100
    assert a[1] == b[1] and a[2] == b[2]
    return out_t, out_r


@pytest.fixture(scope="module")
def c1(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("c1")
    ds = c1_dataset.make(str(d / "data"), oracle, 70_000, 350, 3, num_error_kmers=150_000, genders=["F", "M", "F"])
    prefix = str(d / "bt")
    _cluster(ds["dir"], prefix, 7)
    return ds["dir"], prefix


GIBBS = dict(chains=3, burn=12, samples=30)


@pytest.mark.parametrize("extra_args,env", [((), {}), (("--noise-genotyping",), {}), ((), {"BT_MAX_GROUPS_PER_LAUNCH": "23"}), ((), {"BT_GIBBS_FREE_BYTES": "3000000"}),
                                            ((), {"BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0"})],
                         ids=["default", "noise-genotyping", "23-groups-per-launch", "small-free-bytes", "three-ranks-files"])
def test_c1_text_route_equals_records_route(c1, tmp_path, extra_args, env):
    ds_dir, unit_prefix = c1
    out_t, out_r = _with_and_without(tmp_path, "run", unit_prefix, ds_dir, 7, GIBBS, extra_args, env, ranks="BT_GPUS" in env)
    if "BT_GIBBS_FREE_BYTES" in env:   # the unit was cut into several launches on both routes, the same way: several texts
        cut = [ln.split("] ", 1)[1] for ln in out_t.split("\n") if " launches" in ln and "sampler state" in ln]
        assert cut and cut == [ln.split("] ", 1)[1] for ln in out_r.split("\n") if " launches" in ln and "sampler state" in ln]


def test_sv_rich_ten_samples_text_route_equals_records_route(oracle, tmp_path):
    """SNVs, indels, multi-allelic records, MNVs and blocks of structural variants with nested variants, ten samples (the unit of
    test_genotypes_device_cli_gpu.py's test of the same name)"""
    unit_prefix, ds_dir = sv_rich_unit(oracle, tmp_path)
    _with_and_without(tmp_path, "default", unit_prefix, ds_dir, 11, dict(chains=3, burn=10, samples=25))


def sv_rich_unit(oracle, tmp_path):
    import os

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
    return unit_prefix, str(d)
