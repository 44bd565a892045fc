"""`bayesTyper genotype` with BT_GIBBS_TIMELINE=<file> (the default-mode sampling launches run their stamped kernels, bt_gibbs_timeline_*) against the same
run without the switch: the VCF and both parameter files must be identical; the timeline file holds one parsable object per sampling launch, and the stage
table names the launch."""
import json

import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
from test_candidates_device_cli_gpu import _cluster, _genotype
from test_cli_gpu import _outputs

pytestmark = pytest.mark.gpu

GIBBS = dict(chains=3, burn=12, samples=30)
ROW = "Gibbs timeline, groups "


def test_timeline_switch_changes_no_output(oracle, tmp_path):
    ds = c1_dataset.make(str(tmp_path / "data"), oracle, 40_000, 200, 2, num_error_kmers=80_000, genders=["F", "M"])
    unit_prefix = str(tmp_path / "bt")
    _cluster(ds["dir"], unit_prefix, 7)
    env = {"BT_MAX_GROUPS_PER_LAUNCH": "60"}   # several samplers on the small unit
    tl_file = str(tmp_path / "timeline.jsonl")
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    out_on, err_on = _genotype(on, unit_prefix, ds["dir"], 7, GIBBS, (), dict(env, BT_GIBBS_TIMELINE=tl_file, BT_GIBBS_TIMELINE_RAW="1"))
    out_off, err_off = _genotype(off, unit_prefix, ds["dir"], 7, GIBBS, (), env)
    a, b = _outputs(on), _outputs(off)
    assert a[0] == b[0] and len(a[0]) > 100
    assert a[1] == b[1] and a[2] == b[2]
    assert ROW not in err_off and "BT_GIBBS_TIMELINE" not in out_off + out_on
    objs = [json.loads(line) for line in open(tl_file).read().splitlines()]
    assert len(objs) >= 2
    assert err_on.count(ROW) == len(objs)
    covered = []
    for o in objs:
        s = o["summary"]
        assert s["records"] > 0 and s["unfinished"] == 0 and o["dropped"] == 0 and o["op"] == "run" and o["launch"] == 0
        assert s["peak_live"] >= 1 and 0 < s["makespan_s"] < 60 and 0 <= s["idle_after_median_share"] <= 1
        assert sum(c["wavefronts"] for c in o["classes"]) == s["records"] == len(o["records"])
        assert all(c["kernel"].startswith("gibbs_") and c["unfinished"] == 0 for c in o["classes"])
        assert 1 <= len(o["longest"]) <= 10 and o["longest"][0]["seconds"] == max(x["seconds"] for x in o["longest"])
        covered.append(tuple(o["groups"]))
        assert o["groups"][1] - o["groups"][0] + 1 == o["num_groups"] <= 60
    assert covered == sorted(covered) and all(covered[i][1] < covered[i + 1][0] for i in range(len(covered) - 1))
