"""BT_GIBBS_NIBBLE_SETS: sparse clusters of 3 to 13 haplotypes keep their zero and plus sets as packed words instead of the unordered_set lists, and sample
what the lists sample — the sets' iteration order decides which haplotype an "add zeros" draw picks, so any difference shows in the next sweep's diplotypes.

One batch per sample count: single clusters of 3, 4, 8, 12 and 13 haplotypes (packed), of 14 and 16 (lists: the first sizes past the limit), nested groups
whose root has 8 (packed) and 16 (lists) haplotypes with children of 4 (packed) and 2 (lists: the two-haplotype code is not touched), and a 64-group tile of
clusters of 3 and 4 haplotypes; a haploid and a zero-ploidy sample (NOHAP through hfd_increment).  3 chains x (2 + 6) sweeps.  Everything is word-for-word
equality between the switch on and off, and all clusters exact against the oracle; a second run() on the same samplers continues the chains from the sets
as the first run left them in HBM.

That the packed code ran is read from the sampler (bt_gibbs_sparse_forms: the form every genotyper was constructed with), and from the oracle's traces that
the sets were in use: in clusters of every packed size some sweep leaves a haplotype without an observation — it stays in, or returns to, the zero set,
and only the draw from that set gives it a frequency again.  (A frequency of exactly zero itself is not part of a trace.)"""
import numpy as np
import pytest

import _oracle
from _gibbs_parity import assert_parity

pytestmark = pytest.mark.gpu

KW = dict(seed=53, chains=3, burn=2, iters=6)
SWEEPS = KW["chains"] * (KW["burn"] + KW["iters"])
S_VALUES = (1, 3, 5)
BATCH_SEED = {1: 6101, 3: 6103, 5: 6105}
SETTINGS = (None, "BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_NO_COPIES", "BT_GIBBS_STEPWISE", "BT_GIBBS_SINGLE_KERNEL")
ENVS = ("BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL", "BT_GIBBS_NO_SIMPLE_KERNEL", "BT_GIBBS_PACK", "BT_GIBBS_NO_PACK", "BT_GIBBS_TAIL_WIDTH", "BT_GIBBS_MID_WIDTH",
        "BT_GIBBS_STEPWISE", "BT_GIBBS_NO_COPIES", "BT_GIBBS_NO_TEAMS", "BT_GIBBS_DEBUG", "BT_GIBBS_BULK_SUBSET", "BT_GIBBS_TEAM_APPLY", "BT_GIBBS_NIBBLE_SETS")
PACKED_SIZES = (3, 4, 8, 12, 13)
LISTS, PACKED = 1, 2


def specs():
    nested = [dict(V=3, H=8, kids=[dict(V=2, H=4, shared=2), dict(V=1, H=2, shared=1)]) for _ in range(2)]      # groups 0, 1
    nested += [dict(V=4, H=16, kids=[dict(V=2, H=4, shared=1), dict(V=1, H=2, shared=2)]) for _ in range(2)]    # 2, 3
    single = []
    for V, H in ((2, 3), (2, 4), (3, 8), (4, 12), (4, 13), (4, 14), (4, 16)):
        single += [dict(V=V, H=H, kpa=1, flank=1), dict(V=V, H=H, kpa=2)]
    small = [dict(V=2, H=4, kpa=2) for _ in range(36)] + [dict(V=2, H=3, kpa=1, flank=1) for _ in range(28)]     # a 64-group tile
    return nested + single + small


def make_batch(S):
    from bayestyper_amd import synth

    sp = specs()
    ploidy = np.full((len(sp), S), 2, np.uint8)
    ploidy[0, 0] = 1          # a haploid and a zero-ploidy sample: a nested group, a packed single cluster, a cluster of the 64-group tile
    ploidy[2, 0] = 0
    ploidy[8, 0] = 1
    ploidy[20, 0] = 0
    if S > 1:
        ploidy[0, 1] = 0
        ploidy[2, 1] = 1
        ploidy[8, 1] = 0
        ploidy[20, 1] = 1
    return synth.make_edge_batch(sp, S, seed=BATCH_SEED[S], ploidy=ploidy, gender=[s % 2 for s in range(S)])


def cluster_traces(flat, traces):
    """per cluster of the batch: [sweep, S] diplotype words"""
    out = []
    for t in traces:
        t = np.asarray(t)
        out += [t[:, v, :] for v in range(t.shape[1])]
    assert len(out) == flat["num_clusters"]
    return out


def unobserved_somewhere(H, trace):
    """some sweep of the cluster in which a haplotype of 0 .. H-1 is in no sample's diplotype"""
    for row in np.asarray(trace):
        seen = set((row & 0xFFFF).tolist()) | set((row >> 16).tolist())
        if len(seen & set(range(H))) < H:
            return True
    return False


_CACHE = {}


def case(oracle, S):
    """the batch of a sample count, its tables, and the oracle's results and traces — computed once"""
    if S not in _CACHE:
        flat = make_batch(S)
        luts = _oracle.build_luts(oracle, S)
        og = _oracle.OrcGibbs(oracle, flat, *luts, **KW)
        og.trace_enable(SWEEPS)
        og.run(8)
        goff = flat["group_cluster_off"]
        ro, to = og.results(), [og.trace(g, int(goff[g + 1] - goff[g]), SWEEPS) for g in range(flat["num_groups"])]
        og.close()
        H = np.asarray(flat["num_haplotypes"])
        per = cluster_traces(flat, to)
        for size in PACKED_SIZES:
            assert any(unobserved_somewhere(size, per[c]) for c in np.flatnonzero(H == size)), f"H = {size}: every haplotype observed in every sweep: choose another seed"
        _CACHE[S] = flat, luts, ro, to
    return _CACHE[S]


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def snapshot(ctx, g):
    ctx.sync()
    return g.results(), g.trace(), g.result_words_host(), g.posterior_summary()


def run_twice(ctx, flat, luts, env, on):
    """one schedule, and a second one on the same sampler -> (first, second, forms); the switch is read when the sampler is created"""
    from bayestyper_amd import lib

    env.setenv("BT_GIBBS_NIBBLE_SETS", "1" if on else "0")
    g = lib.Gibbs(ctx, flat, *luts, **KW)
    env.setenv("BT_GIBBS_NIBBLE_SETS", "0" if on else "1")   # a live sampler keeps the form it was built with
    g.trace_enable(SWEEPS)
    g.run()
    first = snapshot(ctx, g)
    forms = g.sparse_forms()
    g.trace_enable(SWEEPS)
    g.run()
    second = snapshot(ctx, g)
    assert np.array_equal(forms, g.sparse_forms())
    g.close()
    env.delenv("BT_GIBBS_NIBBLE_SETS")
    return first, second, forms


def assert_same(a, b):
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k], equal_nan=(k == "stats")), k
    assert len(a[1]) == len(b[1])
    for g, (x, y) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(x, y), f"group {g}: the diplotype traces differ from sweep {np.argwhere((x != y).any(axis=(1, 2)))[:1]}"
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3])


def check_forms(flat, off_forms, on_forms):
    """off: no packed vertex; on: exactly the sparse vertices of 3 .. 13 haplotypes are packed, and every packed size has one"""
    H = np.asarray(flat["num_haplotypes"])
    assert not (off_forms == PACKED).any() and not (off_forms == 0xFFFFFFFF).any()
    assert np.array_equal(off_forms != 0, on_forms != 0)
    small = (H >= 3) & (H <= 13)
    assert np.array_equal(on_forms == PACKED, (on_forms != 0) & small)
    assert np.array_equal(on_forms == LISTS, (on_forms != 0) & ~small)
    for size in PACKED_SIZES:
        assert ((on_forms == PACKED) & (H == size)).any(), f"no sparse cluster of {size} haplotypes: the packed path did not run for that size"
    for size in (2, 14, 16):
        assert ((on_forms == LISTS) & (H == size)).any(), f"no sparse cluster of {size} haplotypes on the lists"


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("S", S_VALUES)
def test_switch_changes_nothing(gpu_ctx, oracle, clean_env, S, setting):
    """traces of every sweep, results, result words and posterior summary with the switch on and off, after one run and after a second; the first run
    against the oracle, all clusters exact; the packed path was taken"""
    flat, luts, ro, to = case(oracle, S)
    if setting:
        clean_env.setenv(setting, "1")
    off1, off2, off_forms = run_twice(gpu_ctx, flat, luts, clean_env, False)
    on1, on2, on_forms = run_twice(gpu_ctx, flat, luts, clean_env, True)
    check_forms(flat, off_forms, on_forms)
    assert_same(off1, on1)
    assert_same(off2, on2)
    for run in (off1, on1):
        for g, (x, y) in enumerate(zip(to, run[1])):
            assert np.array_equal(x, y[: len(x)]), f"group {g}: the trace diverges from the oracle's"
        assert assert_parity(flat, ro, run[0], KW["chains"] * KW["iters"]) == flat["num_clusters"]
