"""The launch timeline (bt_gibbs_timeline_*): the stamped siblings of the four sampling kernels compute what the unstamped kernels compute, and
their records — one per wavefront of a launch — agree with the host's plan of the launch.

The batch is the smallest that still gives a simple class (two-haplotype clusters), a hot class (H = 8 single clusters and nested groups) and tiles
with lockstep copies, and classes of several workgroups: 58 groups, S = 3, chains=2, burn=3, iters=5."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import _oracle

pytestmark = pytest.mark.gpu

S = 3
KW = dict(seed=17, chains=2, burn=3, iters=5)
SWEEPS = KW["chains"] * (KW["burn"] + KW["iters"])
KERNEL_ENVS = ("BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL", "BT_GIBBS_NO_SIMPLE_KERNEL", "BT_GIBBS_PACK")
KERNEL_ID = {"generic": 0, "hot": 1, "simple": 2, "single": 3}   # BT_GIBBS_DEBUG's names -> bt_gibbs_timeline_record::kernel


def V_of(H):
    return max(1, int(np.ceil(np.log2(H))))


@pytest.fixture(scope="module")
def batch(oracle):
    from bayestyper_amd import synth

    # (a tile of two-haplotype clusters runs the simple sweep when it is 64 lanes wide: more than 32 such groups;
    # and a class with more than one workgroup: 16 single clusters of H = 8 fill a tile, nested groups go four to a tile)
    specs = ([dict(V=1, H=2, kpa=2, flank=1) for _ in range(34)] + [dict(V=V_of(8), H=8, kpa=1, flank=1) for _ in range(18)] +
             [dict(V=V_of(8), H=8, kids=[dict(V=2, H=4)]) for _ in range(6)])
    flat = synth.make_edge_batch(specs, S, seed=1234)
    return flat, _oracle.build_luts(oracle, S)


@pytest.fixture
def clean_env(monkeypatch):
    for k in KERNEL_ENVS + ("BT_GIBBS_TAIL_WIDTH", "BT_GIBBS_STEPWISE", "BT_GIBBS_NO_PACK", "BT_GIBBS_DEBUG"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def run_once(ctx, batch, timeline=0):
    """bt_gibbs_run with the diplotype trace on -> (results, traces, timeline or None, host seconds around run + sync)"""
    from bayestyper_amd import lib

    flat, luts = batch
    g = lib.Gibbs(ctx, flat, *luts, **KW)
    g.trace_enable(SWEEPS)
    if timeline:
        g.timeline_enable(timeline)
    ctx.sync()
    t0 = time.perf_counter()
    g.run()
    ctx.sync()
    dt = time.perf_counter() - t0
    tl = None
    if timeline:
        tl = g.timeline() + (g.timeline_sizes(),)
    r, t = g.results(), g.trace()
    g.close()
    return r, t, tl, dt


def assert_same(a, b):
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k], equal_nan=(k == "stats")), k
    assert len(a[1]) == len(b[1])
    for g, (x, y) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(x, y), g


@pytest.fixture(scope="module")
def unstamped(gpu_ctx, batch):
    """the reference of the module: the run with the timeline off (no kernel-selection variable set)"""
    import os

    assert not any(os.environ.get(k) for k in KERNEL_ENVS)
    return run_once(gpu_ctx, batch)


def check_launch(rec, launch, num_groups):
    """the records of one launch against the plan: tiles 0..T-1 without a gap, every tile's waves 0..w-1 exactly once, the groups add up"""
    r = rec[rec["launch"] == launch]
    assert len(r) > 0
    tiles = np.unique(r["tile"])
    assert np.array_equal(tiles, np.arange(len(tiles))), tiles
    groups = 0
    for t in tiles:
        rt = r[r["tile"] == t]
        assert sorted(rt["wave"].tolist()) == list(range(len(rt))), (t, rt["wave"])
        assert len(set(rt["groups"].tolist())) == 1 and len(set(rt["launch_class"].tolist())) == 1 and len(set(rt["lds_bytes"].tolist())) == 1
        groups += int(rt["groups"][0])
    assert groups == num_groups
    assert (r["start_tick"] > 0).all() and (r["start_tick"] <= r["end_tick"]).all()
    return r


def test_results_bit_equal_and_one_launch(gpu_ctx, batch, unstamped, clean_env):
    from bayestyper_amd import lib

    r, t, (rec, khz, dropped, sizes), dt = run_once(gpu_ctx, batch, timeline=4)
    assert_same(unstamped, (r, t))
    assert sizes[1] == 1 and dropped == 0 and sizes[2] == 0 and sizes[0] == len(rec) and khz == sizes[3] and khz > 0
    one = check_launch(rec, 0, batch[0]["num_groups"])
    assert len(one) == len(rec) and (rec["op"] == 0).all()
    span_ms = (int(one["end_tick"].max()) - int(one["start_tick"].min())) / khz
    print(f"launch span {span_ms:.3f} ms, host bracket {dt * 1e3:.3f} ms, {len(rec)} wavefronts, kernels {sorted(set(rec['kernel'].tolist()))}")
    assert span_ms <= dt * 1e3 + 1.0
    assert {2, 1} <= set(rec["kernel"].tolist())   # a simple class and a hot class
    assert len(np.unique(rec["tile"])) >= 4
    s = lib.timeline_summary(rec, launch=0)
    assert s["records"] == len(rec) and s["unfinished"] == 0 and 1 <= s["peak_live"] <= len(rec)
    assert s["busy_ticks"] == int((rec["end_tick"] - rec["start_tick"]).sum())


@pytest.mark.parametrize("env", [None, "BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL", "BT_GIBBS_NO_SIMPLE_KERNEL", "BT_GIBBS_PACK"])
def test_kernel_kinds(gpu_ctx, batch, unstamped, clean_env, capfd, env):
    if env:
        clean_env.setenv(env, "1")
    base = run_once(gpu_ctx, batch) if env else unstamped
    clean_env.setenv("BT_GIBBS_DEBUG", "1")
    capfd.readouterr()
    r, t, (rec, khz, dropped, sizes), _ = run_once(gpu_ctx, batch, timeline=1)
    err = capfd.readouterr().err
    clean_env.delenv("BT_GIBBS_DEBUG")
    assert_same(base, (r, t))
    assert_same(unstamped, (r, t))   # (the kernel-selection variables change nothing either)
    named = {int(m.group(1)): m.group(2) for m in re.finditer(r"bt_gibbs: class (\d+) kernel=(\w+):", err)}
    assert named, err
    assert sizes[1] == 1 and dropped == 0
    check_launch(rec, 0, batch[0]["num_groups"])
    assert set(rec["launch_class"].tolist()) == set(named)
    for c, name in named.items():
        assert set(rec["kernel"][rec["launch_class"] == c].tolist()) == {KERNEL_ID[name]}, (c, name)
    kinds = set(named.values())
    if env == "BT_GIBBS_NO_HOT_KERNEL":
        assert "generic" in kinds and not kinds & {"hot", "single"}
    elif env == "BT_GIBBS_SINGLE_KERNEL":
        assert "single" in kinds
    elif env == "BT_GIBBS_NO_SIMPLE_KERNEL":
        assert "simple" not in kinds
    else:
        assert {"simple", "hot"} <= kinds


def stepwise(ctx, batch, timeline):
    from bayestyper_amd import lib

    flat, luts = batch
    g = lib.Gibbs(ctx, flat, *luts, **KW)
    if timeline is not None:
        g.timeline_enable(timeline)
    g.init_chain(0)
    g.sweep(4, 1)
    ctx.sync()
    return g


def test_two_launches_capacity_and_errors(gpu_ctx, batch, clean_env):
    from bayestyper_amd import lib

    g0 = stepwise(gpu_ctx, batch, None)
    want = g0.results()
    assert g0.timeline_sizes()[:3] == (0, 0, 0) and len(g0.timeline()[0]) == 0
    bytes_off = g0.device_bytes()
    g0.close()
    # room for both launches: the same set of (tile, wave) in each
    g = stepwise(gpu_ctx, batch, 2)
    assert g.device_bytes() > bytes_off
    rec, khz, dropped = g.timeline()
    assert g.timeline_sizes()[1:3] == (2, 0) and dropped == 0
    a, b = check_launch(rec, 0, batch[0]["num_groups"]), check_launch(rec, 1, batch[0]["num_groups"])
    assert set(zip(a["tile"].tolist(), a["wave"].tolist())) == set(zip(b["tile"].tolist(), b["wave"].tolist())) and len(a) == len(b)
    assert (a["op"] == 1).all() and (b["op"] == 2).all()
    assert int(a["end_tick"].max()) <= int(b["start_tick"].min())   # the launches of one stream run one after the other
    got = g.results()
    for k in want:
        assert np.array_equal(want[k], got[k], equal_nan=(k == "stats")), k
    # a capacity one short: an error, nothing written
    n = len(rec)
    buf = np.full(n, 0xAB, np.uint8).repeat(48).view(lib.TIMELINE_RECORD)
    before = buf.copy()
    cnt = C.c_uint64()
    assert lib.bt_gibbs_timeline_fetch(g.h, buf.ctypes.data, n - 1, C.byref(cnt)) != 0
    assert b"too small" in lib.bt_last_error() and cnt.value == n and np.array_equal(buf.view(np.uint8), before.view(np.uint8))
    # off: nothing to fetch, the buffer is released
    g.timeline_enable(0)
    assert g.timeline_sizes()[:3] == (0, 0, 0) and len(g.timeline()[0]) == 0 and g.device_bytes() == bytes_off
    g.close()
    # room for one launch: the second runs unstamped and is counted
    g = stepwise(gpu_ctx, batch, 1)
    rec, _, dropped = g.timeline()
    assert g.timeline_sizes()[1:3] == (1, 1) and dropped == 1 and set(rec["launch"].tolist()) == {0}
    check_launch(rec, 0, batch[0]["num_groups"])
    got = g.results()
    for k in want:
        assert np.array_equal(want[k], got[k], equal_nan=(k == "stats")), k
    g.close()


def test_noise_chain_is_not_recorded(gpu_ctx, batch, oracle, clean_env):
    """a resident noise chain on a sampler whose timeline is on: the histograms of a sampler without it, and no record added"""
    from bayestyper_amd import lib

    flat, luts = batch
    kw = dict(seed=5, chains=1, burn=1, iters=2, noise_seeding=1)
    hists = []
    for timeline in (0, 8):
        g = lib.Gibbs(gpu_ctx, flat, *luts, **kw)
        if timeline:
            g.timeline_enable(timeline)
        g.set_noise_lut(luts[1])
        g.init_chain(0)
        sizes0 = g.timeline_sizes()
        assert g.noise_chain_begin(3, 1), "the batch should fit the GPU as one resident launch"
        if timeline:   # the stream-enqueuing calls are rejected while the chain's launch is (or may be) resident
            h = [g.noise_chain_step(None), g.noise_chain_step(None)]
            with pytest.raises(lib.BtError, match=r"bt_gibbs_timeline_fetch: a resident noise chain is in progress"):
                g.timeline()
            with pytest.raises(lib.BtError, match=r"bt_gibbs_timeline_enable: a resident noise chain is in progress"):
                g.timeline_enable(2)
            h.append(g.noise_chain_step(None))
        else:
            h = [g.noise_chain_step(None) for _ in range(3)]
        g.noise_chain_end()
        gpu_ctx.sync()
        if timeline:
            assert sizes0[1:3] == (1, 0) and g.timeline_sizes() == sizes0
            rec = g.timeline()[0]
            assert set(rec["launch"].tolist()) == {0} and (rec["op"] == 1).all()
        hists.append((np.stack(h), g.results()))
        g.close()
    assert hists[0][0].sum() > 0 and np.array_equal(hists[0][0], hists[1][0])
    for k in hists[0][1]:
        assert np.array_equal(hists[0][1][k], hists[1][1][k], equal_nan=(k == "stats")), k
