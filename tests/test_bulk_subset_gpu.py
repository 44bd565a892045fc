"""BT_GIBBS_BULK_SUBSET: a chain start that draws the k-mer subset across a group's lockstep copies computes what the sequential chain start computes.

One batch of 82 groups at S = 3 in which tiles with 16 copies (nested groups, a 16-candidate cluster), with 4 copies (8-candidate single clusters) and
64-group tiles (two-, three- and four-candidate clusters) all occur; one cluster of each narrow kind has more than 312 unique k-mers (its draws cross a
generator block), a nested child has no unique k-mer at all, and the nested groups share multicluster k-mers.  3 chains x (2 + 3) sweeps: the second
and third chain start from the generator the chain before left behind.  Everything is word-for-word equality between the switch on and off, and the
usual parity with the oracle."""
import numpy as np
import pytest

import _oracle
from _gibbs_parity import assert_parity

pytestmark = pytest.mark.gpu

S = 3
KW = dict(seed=31, chains=3, burn=2, iters=3)
SWEEPS = KW["chains"] * (KW["burn"] + KW["iters"])
KERNEL_ENVS = ("BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL", "BT_GIBBS_NO_SIMPLE_KERNEL", "BT_GIBBS_PACK")


def specs():
    nested = [dict(V=3, H=8, kids=[dict(V=2, H=4, shared=2)]) for _ in range(5)]
    nested.append(dict(V=3, H=8, kpa=60, flank=3, kids=[dict(V=2, H=4, shared=3)]))    # 363 unique k-mers in a 16-copy tile
    nested.append(dict(V=3, H=8, kids=[dict(V=1, H=2, kpa=0, shared=4)]))              # a child of multicluster k-mers only: nu = 0
    wide = [dict(V=4, H=16, kpa=2, flank=1)]                                            # a single cluster in a four-group tile
    mid = [dict(V=3, H=8, kpa=1, flank=1) for _ in range(17)] + [dict(V=3, H=8, kpa=55, flank=2)]   # 16 to a tile, four copies; one of 332 unique k-mers
    small = [dict(V=2, H=4, kpa=2) for _ in range(12)] + [dict(V=2, H=3, kpa=1, flank=1) for _ in range(8)]
    two = [dict(V=1, H=2, kpa=2, flank=1) for _ in range(36)]
    return nested + wide + mid + small + two


@pytest.fixture(scope="module")
def batch(oracle):
    from bayestyper_amd import synth

    flat = synth.make_edge_batch(specs(), S, seed=4321)
    nu = np.diff(flat["unique_off"].astype(np.int64))
    nm = np.diff(flat["multi_off"].astype(np.int64))
    assert (nu > 312).sum() >= 2 and (nu == 0).any() and (nm > 0).any()
    return flat, _oracle.build_luts(oracle, S)


@pytest.fixture
def clean_env(monkeypatch):
    for k in KERNEL_ENVS + ("BT_GIBBS_TAIL_WIDTH", "BT_GIBBS_MID_WIDTH", "BT_GIBBS_STEPWISE", "BT_GIBBS_NO_PACK", "BT_GIBBS_NO_COPIES", "BT_GIBBS_DEBUG", "BT_GIBBS_BULK_SUBSET"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def run_once(ctx, batch, env, bulk):
    """one schedule -> (results, traces, result words, posterior summary); the switch is read when the sampler is created"""
    from bayestyper_amd import lib

    flat, luts = batch
    env.setenv("BT_GIBBS_BULK_SUBSET", "1" if bulk else "0")
    g = lib.Gibbs(ctx, flat, *luts, **KW)
    env.delenv("BT_GIBBS_BULK_SUBSET")
    g.trace_enable(SWEEPS)
    g.run()
    ctx.sync()
    out = g.results(), g.trace(), g.result_words_host(), g.posterior_summary()
    g.close()
    return out


def assert_same(a, b):
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k], equal_nan=(k == "stats")), k
    assert len(a[1]) == len(b[1])
    for g, (x, y) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(x, y), f"group {g}: the diplotype traces differ from sweep {np.argwhere((x != y).any(axis=(1, 2)))[:1]}"
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3])


@pytest.fixture(scope="module")
def oracle_run(oracle, batch):
    """the oracle's results and traces of the batch, computed once"""
    flat, luts = batch
    og = _oracle.OrcGibbs(oracle, flat, *luts, **KW)
    og.trace_enable(SWEEPS)
    og.run(8)
    goff = flat["group_cluster_off"]
    out = og.results(), [og.trace(g, int(goff[g + 1] - goff[g]), SWEEPS) for g in range(flat["num_groups"])]
    og.close()
    return out


def test_tiles_of_every_kind(gpu_ctx, batch, clean_env, capfd):
    """the batch does give tiles with 16 copies, with 4 copies and 64-group tiles (the plan, as BT_GIBBS_DEBUG prints it)"""
    import re

    from bayestyper_amd import lib

    clean_env.setenv("BT_GIBBS_DEBUG", "1")
    capfd.readouterr()
    g = lib.Gibbs(gpu_ctx, batch[0], *batch[1], **KW)
    g.close()
    err = capfd.readouterr().err
    copies = {int(m) for m in re.findall(r"copies[= ](\d+)", err)}
    print(err)
    assert {1, 4, 16} <= copies, err


@pytest.mark.parametrize("env", [None, "BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL"])
def test_switch_changes_nothing(gpu_ctx, batch, oracle_run, clean_env, env):
    """hot, general and single kernels: traces of every sweep, results, result words and posterior summary with the switch on and off; and the oracle"""
    if env:
        clean_env.setenv(env, "1")
    off = run_once(gpu_ctx, batch, clean_env, False)
    on = run_once(gpu_ctx, batch, clean_env, True)
    assert_same(off, on)
    flat = batch[0]
    ro, to = oracle_run
    for g, (x, y) in enumerate(zip(to, on[1])):
        assert np.array_equal(x, y[: len(x)]), f"group {g}: the trace diverges from the oracle's"
    exact = assert_parity(flat, ro, on[0], KW["chains"] * KW["iters"])
    assert exact == flat["num_clusters"]
