"""BT_GIBBS_TEAM_APPLY: a visit whose per-sample bookkeeping is dealt to the teams and copies of a narrow tile's group — the shared multiplicities and the
version bump of a round's picks on the team that drew the sample, the deferral test of a collected sweep and prepare_nested on copy s of sample s, the
non-zero scan and the zero-set reset over the haplotypes — computes what the visit that replays all of it on every copy computes.

One batch per sample count in which tiles with 16 copies (nested groups with one and with three children, a 16-candidate cluster), with 4 copies
(8-candidate clusters) and 64-group tiles (two- to four-candidate clusters) all occur.  A child has no unique k-mer, one group's shared k-mers have
multiplicity 2 in the root and an intercluster copy, one shared k-mer has a zero count in the first sample alone (the `mcn == 0` branches), and two
nested groups hold a haploid and a zero-ploidy sample (NOHAP through the team path).  S = 1: no teams, the deferral test still dealt; S = 2, 3;
S = 5: four-copy tiles draw in teams of four, a second, partial round; S = 17: two rounds on 16-copy tiles too, and two rounds of the dealt tests.
3 chains x (2 + 6) sweeps.  Everything is word-for-word equality between the switch on and off, and all clusters exact against the oracle."""
import re

import numpy as np
import pytest

import _oracle
from _gibbs_parity import assert_parity

pytestmark = pytest.mark.gpu

KW = dict(seed=47, chains=3, burn=2, iters=6)
SWEEPS = KW["chains"] * (KW["burn"] + KW["iters"])
S_VALUES = (1, 2, 3, 5, 17)
BATCH_SEED = {1: 5101, 2: 5102, 3: 5103, 5: 5105, 17: 5117}
# kernel settings: default, the same code with the hot arrays in HBM, no teams, no copies (the switch then changes nothing, trivially), stepwise driving
SETTINGS = (None, "BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_NO_TEAMS", "BT_GIBBS_NO_COPIES", "BT_GIBBS_STEPWISE")
ENVS = ("BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL", "BT_GIBBS_NO_SIMPLE_KERNEL", "BT_GIBBS_PACK", "BT_GIBBS_NO_PACK", "BT_GIBBS_TAIL_WIDTH", "BT_GIBBS_MID_WIDTH",
        "BT_GIBBS_STEPWISE", "BT_GIBBS_NO_COPIES", "BT_GIBBS_NO_TEAMS", "BT_GIBBS_DEBUG", "BT_GIBBS_BULK_SUBSET", "BT_GIBBS_TEAM_APPLY")
N_NESTED = 8


def specs():
    one = dict(V=2, H=4, shared=2)
    nested = [dict(V=3, H=8, kids=[dict(one)]) for _ in range(4)]                                          # groups 0-3: one child
    nested += [dict(V=3, H=8, kids=[dict(one), dict(V=2, H=4, shared=1), dict(V=1, H=2, shared=3)]) for _ in range(2)]   # 4, 5: three children
    nested.append(dict(V=3, H=8, kids=[dict(V=1, H=2, kpa=0, shared=4)]))                                  # 6: a child of multicluster k-mers only
    nested.append(dict(V=3, H=8, kids=[dict(one)], shared_mult=(2, 1), shared_ic=(1, 1)))                  # 7
    assert len(nested) == N_NESTED
    wide = [dict(V=4, H=16, kpa=2, flank=1)]                                                               # a single cluster in a four-group tile (nm == 0)
    mid = [dict(V=3, H=8, kpa=1, flank=1) for _ in range(12)]                                              # four copies
    small = [dict(V=2, H=4, kpa=2) for _ in range(36)] + [dict(V=2, H=3, kpa=1, flank=1) for _ in range(6)] + [dict(V=1, H=2, kpa=2, flank=1) for _ in range(4)]   # a 64-group tile (more than 32 lanes: no copies)
    return nested + wide + mid + small


def make_batch(S):
    from bayestyper_amd import synth

    sp = specs()
    ploidy = np.full((len(sp), S), 2, np.uint8)
    ploidy[1, 0] = 1          # a haploid and a zero-ploidy sample in nested groups
    ploidy[5, 0] = 0
    if S > 1:
        ploidy[1, 1] = 0
        ploidy[5, 1] = 1
    # the root's first shared k-mer (row 2 * V * kpa, after its allele k-mers): unobserved in the first sample alone
    counts = {(g, 0, 6): [0] + [9 + (s % 5) for s in range(1, S)] for g in (0, 4)}
    return synth.make_edge_batch(sp, S, seed=BATCH_SEED[S], ploidy=ploidy, gender=[s % 2 for s in range(S)], counts=counts)


def changing_roots(traces):
    """nested groups whose root diplotype changes between two consecutive collected sweeps of a chain for some sample"""
    per = KW["burn"] + KW["iters"]
    n = 0
    for g in range(N_NESTED):
        t = np.asarray(traces[g])[:, 0, :]
        moved = False
        for ch in range(KW["chains"]):
            col = t[ch * per + KW["burn"]:(ch + 1) * per]
            moved = moved or bool((col[1:] != col[:-1]).any())
        n += int(moved)
    return n


_CACHE = {}


def case(oracle, S):
    """the batch of a sample count, its tables, and the oracle's results and traces — computed once"""
    if S not in _CACHE:
        flat = make_batch(S)
        nm = np.diff(flat["multi_off"].astype(np.int64))
        nu = np.diff(flat["unique_off"].astype(np.int64))
        assert (nm > 0).any() and (nu == 0).any()
        luts = _oracle.build_luts(oracle, S)
        og = _oracle.OrcGibbs(oracle, flat, *luts, **KW)
        og.trace_enable(SWEEPS)
        og.run(8)
        goff = flat["group_cluster_off"]
        ro, to = og.results(), [og.trace(g, int(goff[g + 1] - goff[g]), SWEEPS) for g in range(flat["num_groups"])]
        og.close()
        assert 2 * changing_roots(to) >= N_NESTED, "the oracle's nested roots hardly move: choose another seed"
        _CACHE[S] = flat, luts, ro, to
    return _CACHE[S]


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def run_once(ctx, flat, luts, env, on):
    """one schedule -> (results, traces, result words, posterior summary); the switch is read when the sampler is created"""
    from bayestyper_amd import lib

    env.setenv("BT_GIBBS_TEAM_APPLY", "1" if on else "0")
    g = lib.Gibbs(ctx, flat, *luts, **KW)
    env.delenv("BT_GIBBS_TEAM_APPLY")
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


def check(ctx, env, flat, luts, ro, to):
    off = run_once(ctx, flat, luts, env, False)
    on = run_once(ctx, flat, luts, env, True)
    assert_same(off, on)
    for g, (x, y) in enumerate(zip(to, on[1])):
        assert np.array_equal(x, y[: len(x)]), f"group {g}: the trace diverges from the oracle's"
    assert assert_parity(flat, ro, on[0], KW["chains"] * KW["iters"]) == flat["num_clusters"]


@pytest.mark.parametrize("S", S_VALUES)
def test_tiles_of_every_kind(gpu_ctx, oracle, clean_env, capfd, S):
    """the batch does give tiles with 16 copies, with 4 copies and 64-group tiles (the plan, as BT_GIBBS_DEBUG prints it)"""
    from bayestyper_amd import lib

    flat, luts = case(oracle, S)[:2]
    clean_env.setenv("BT_GIBBS_DEBUG", "1")
    capfd.readouterr()
    g = lib.Gibbs(gpu_ctx, flat, *luts, **KW)
    g.close()
    err = capfd.readouterr().err
    copies = {int(m) for m in re.findall(r"copies[= ](\d+)", err)}
    print(err)
    assert {1, 4, 16} <= copies, err


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("S", S_VALUES)
def test_switch_changes_nothing(gpu_ctx, oracle, clean_env, S, setting):
    """traces of every sweep, results, result words and posterior summary with the switch on and off; and the oracle, all clusters exact"""
    flat, luts, ro, to = case(oracle, S)
    if setting:
        clean_env.setenv(setting, "1")
    check(gpu_ctx, clean_env, flat, luts, ro, to)


@pytest.mark.parametrize("setting", (None, "BT_GIBBS_NO_HOT_KERNEL"))
def test_bench_nested_shape(gpu_ctx, oracle, clean_env, setting):
    """the bench's own nested shape: eight heterogeneous groups of class C at S = 3"""
    from bayestyper_amd import synth

    flat = synth.make_hetero_batch("C", 8, 3, 7301)
    luts = _oracle.build_luts(oracle, 3)
    og = _oracle.OrcGibbs(oracle, flat, *luts, **KW)
    og.trace_enable(SWEEPS)
    og.run(8)
    goff = flat["group_cluster_off"]
    ro, to = og.results(), [og.trace(g, int(goff[g + 1] - goff[g]), SWEEPS) for g in range(flat["num_groups"])]
    og.close()
    if setting:
        clean_env.setenv(setting, "1")
    check(gpu_ctx, clean_env, flat, luts, ro, to)
