"""The Gibbs sampler at the boundaries of the tile builder's decisions and at numeric edges.  Every case runs the GPU sampler and the oracle
(oracle/oracle_gibbs.cpp) on the same batch — synth.make_edge_batch: groups of exactly the dimensions asked for —, seed and tables, and asserts
bit-equal diplotype traces over the traced sweeps and identical sampling frequencies for every cluster (assert_parity: exact == clusters).

With BT_GIBBS_DEBUG set, bt_gibbs_create prints every launch class's kernel and the distinct set-ups of its tiles (the table of unique-k-mer
sums: tagged = the direct-mapped cache, whole = a dense table rebuilt whole when cleared, invalidated = one invalidated block-wise by its tile,
wide = one invalidated by the whole GPU between noise iterations; teams; copies; the per-sample cache length scache_n).  Each case asserts from
that output that it reached the path it is named after."""
import re

import numpy as np
import pytest

import _oracle
from _gibbs_parity import assert_parity

pytestmark = pytest.mark.gpu

KERNEL_ENVS = ("BT_GIBBS_NO_HOT_KERNEL", "BT_GIBBS_SINGLE_KERNEL", "BT_GIBBS_NO_SIMPLE_KERNEL")


def setups(err):
    """the tile set-ups BT_GIBBS_DEBUG printed: one dict per distinct set-up of a launch class (+ the class's kernel)"""
    out = []
    for line in err.splitlines():
        m = re.match(r"bt_gibbs: class \d+ kernel=(\w+):(.*)", line)
        if m:
            for body in re.findall(r"\[([^\]]+)\]", m.group(2)):
                d = {k: (v if k == "table" else int(v)) for k, v in (kv.split("=") for kv in body.split())}
                d["kernel"] = m.group(1)
                out.append(d)
    return out


@pytest.fixture
def debug(monkeypatch, capfd):
    """-> read(): the tile set-ups of the samplers created since the last call; no kernel-selection variable is set"""
    for k in KERNEL_ENVS + ("BT_GIBBS_TAIL_WIDTH",):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BT_GIBBS_DEBUG", "1")
    capfd.readouterr()
    return lambda: setups(capfd.readouterr().err)


def V_of(H):
    return max(1, int(np.ceil(np.log2(H))))


def single(H, **kw):
    return dict(V=V_of(H), H=H, **kw)


def nested(H, kids=((2, 4),), **kw):
    return dict(V=V_of(H), H=H, kids=[dict(V=v, H=h) for v, h in kids], **kw)


def gpu_run(gpu_ctx, flat, luts, sweeps, **kw):
    from bayestyper_amd import lib

    g = lib.Gibbs(gpu_ctx, flat, *luts, **kw)
    g.trace_enable(sweeps)
    g.run()
    gpu_ctx.sync()
    r, t = g.results(), g.trace()
    g.close()
    return r, t


def run_pair(gpu_ctx, oracle, flat, luts=None, **kw):
    """bt_gibbs_run against the oracle's run: the traces of every sweep of every chain bit-equal, the frequencies identical -> (GPU results, traces)"""
    luts = luts if luts is not None else _oracle.build_luts(oracle, flat["S"])
    sweeps = kw["chains"] * (kw["burn"] + kw["iters"])
    og = _oracle.OrcGibbs(oracle, flat, *luts, **kw)
    og.trace_enable(sweeps)
    og.run(8)
    ro = og.results()
    goff = flat["group_cluster_off"]
    to = [og.trace(g, int(goff[g + 1] - goff[g]), sweeps) for g in range(flat["num_groups"])]
    og.close()
    rg, tg = gpu_run(gpu_ctx, flat, luts, sweeps, **kw)
    for g in range(flat["num_groups"]):
        assert len(to[g]) == sweeps
        same = (to[g] == tg[g][:sweeps]).all(axis=(1, 2))
        assert same.all(), f"group {g}: diplotype trace diverges at sweep {int(np.argmin(same))}"
    assert_exact_parity(flat, ro, rg, kw["chains"] * kw["iters"])
    return rg, tg


def assert_exact_parity(flat, ro, rg, n_collect):
    """assert_parity with exact == every cluster.  Allele statistics over a wrapped multiplicity of 0 are NaN / inf (a division by it): those
    entries must sit at the same places and be equal; assert_parity compares the others"""
    so, sg = ro["stats"], rg["stats"]
    assert so.shape == sg.shape and np.array_equal(np.isnan(so), np.isnan(sg)) and np.array_equal(so[np.isinf(so)], sg[np.isinf(so)])
    ro, rg = dict(ro, stats=np.where(np.isnan(so), 0.0, so)), dict(rg, stats=np.where(np.isnan(sg), 0.0, sg))
    assert assert_parity(flat, ro, rg, n_collect) == flat["num_clusters"]


def run_noise_loop(gpu_ctx, oracle, flat, luts, noise_tables, n_it=8, seed=5):
    """The noise drivers' stepwise use of a sampler (InferenceEngine.cpp:60-98): per chain init_chain, then per iteration one sweep and the noise
    counts — which clear every genotyper's tables (clearGenotyperCache: a dense table rebuilt whole, invalidated by its tile or by the whole GPU, the
    tagged cache emptied) — and a new noise table every other iteration; the histogram of every iteration, every sweep's diplotypes and the
    collected results against the oracle.  -> the number of noise k-mers tallied"""
    from bayestyper_amd import lib

    first = n_it // 2
    kw = dict(seed=seed, chains=2, burn=first, iters=n_it - first, noise_seeding=1)
    og = _oracle.OrcGibbs(oracle, flat, *luts, **kw)
    gg = lib.Gibbs(gpu_ctx, flat, *luts, **kw)
    og.trace_enable(2 * n_it)
    gg.trace_enable(2 * n_it)
    tally = 0
    for chain in range(2):
        og.init_chain(chain)
        gg.init_chain(chain)
        for it in range(n_it):
            og.sweep(1, it >= first)
            gg.sweep(1, it >= first)
            ho, hg = og.noise_counts(), gg.noise_counts()
            assert np.array_equal(ho, hg), (chain, it)
            tally += int(ho.sum())
            if it % 2 == 1:
                ln = noise_tables[(chain * n_it + it) % len(noise_tables)]
                og.set_noise_lut(ln)
                gg.set_noise_lut(ln)
        if chain == 0:   # estimateNoise deletes the genotypers after every chain
            og.reset_groups()
            gg.reset_groups()
    gpu_ctx.sync()
    ro, rg = og.results(), gg.results()
    goff = flat["group_cluster_off"]
    tg = gg.trace()
    for g in range(flat["num_groups"]):
        to = og.trace(g, int(goff[g + 1] - goff[g]), 2 * n_it)
        assert len(to) == 2 * n_it and np.array_equal(to, tg[g][: len(to)]), f"group {g}"
    og.close()
    gg.close()
    assert_exact_parity(flat, ro, rg, n_it - first)   # (the first chain's samples went with its genotypers)
    return tally


def check_kernel_paths(gpu_ctx, flat, luts, base, monkeypatch, debug, **kw):
    """(f) the same run with each kernel-selection variable: bit-equal results and traces, and the launch classes show the kernel was (not) used"""
    sweeps = kw["chains"] * (kw["burn"] + kw["iters"])
    for env in KERNEL_ENVS:
        monkeypatch.setenv(env, "1")
        r, t = gpu_run(gpu_ctx, flat, luts, sweeps, **kw)
        monkeypatch.delenv(env)
        kernels = {d["kernel"] for d in debug()}
        if env == "BT_GIBBS_NO_HOT_KERNEL":
            assert "generic" in kernels and not kernels & {"hot", "single"}, kernels
        elif env == "BT_GIBBS_SINGLE_KERNEL":
            assert "single" in kernels, kernels
        else:
            assert "simple" not in kernels, kernels
        for k in base[0]:
            assert np.array_equal(base[0][k], r[k], equal_nan=(k == "stats")), (env, k)
        for g, (a, b) in enumerate(zip(base[1], t)):
            assert np.array_equal(a, b), (env, g)


# --------------------------------------------------------------------------------------------------------------------------------------
# (a) haplotype counts: one cluster per group.  Per H enough groups for tiles of that H alone (64-wide tiles below 6 candidates, 16-wide
#     up to 15, 4-wide above; one group per tile where S x (H(H+1)/2 + H) > 65 536), so every tile's Hm — and with it HWm = ceil(Hm / 32),
#     Bcap, Dcm — is the edge value
# --------------------------------------------------------------------------------------------------------------------------------------
A_H = (2, 3, 4, 5, 9, 10, 31, 32, 33, 63, 64, 65, 128, 129, 255, 256)


def haplotype_batch(S, Hs, seed, per_h=None):
    from bayestyper_amd import synth

    n_of = per_h or (lambda H: 64 if H < 6 else (16 if H < 16 else 4))
    specs = [single(H, kpa=1, flank=1, ic_kmers=1) for H in Hs for _ in range(n_of(H))]
    return synth.make_edge_batch(specs, S, seed)


@pytest.mark.parametrize("S", [1, 3, 30])
def test_haplotype_count_sweep(gpu_ctx, oracle, debug, monkeypatch, S):
    if S == 30:
        Hs = (33, 129, 256)
        flat = haplotype_batch(S, Hs, seed=930, per_h=lambda H: 4 if H < 64 else (2 if H < 200 else 1))
        kw = dict(seed=31, chains=2, burn=2, iters=3)
    else:
        Hs = A_H
        flat = haplotype_batch(S, Hs, seed=900 + S)
        kw = dict(seed=11 + S, chains=2, burn=3, iters=4)
    base = run_pair(gpu_ctx, oracle, flat, **kw)
    seen = debug()
    assert {d["Hm"] for d in seen} == set(Hs)   # every H has tiles of its own
    kern = {d["Hm"]: d["kernel"] for d in seen}
    if S != 30:
        assert kern[2] == "simple" and kern[3] == "hot" and kern[10] == "hot", kern
    if S == 3:   # (f) the kernel-selection variables change nothing
        check_kernel_paths(gpu_ctx, flat, _oracle.build_luts(oracle, S), base, monkeypatch, debug, **kw)


# --------------------------------------------------------------------------------------------------------------------------------------
# (b) tile widths, copies and teams: 1 .. 65 groups of small clusters (H = 3..8: 64-wide tiles below 6 candidates, 16-wide from 6 on); a
#     partial tile of n groups is padded to a power of two and its idle lanes run 64 / width copies, which work in teams of min(S, copies) when
#     the table is dense and S > 1
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 5, 30])
def test_tile_widths_copies_and_teams(gpu_ctx, oracle, debug, S):
    from bayestyper_amd import synth

    seen = []
    for n in (1, 3, 4, 5, 16, 17, 33, 64, 65):
        rng = np.random.default_rng(50 + n)
        specs = [single(int(rng.integers(3, 9)), kpa=1, flank=int(rng.integers(0, 3))) for _ in range(n)]
        flat = synth.make_edge_batch(specs, S, seed=700 + 10 * S + n)
        run_pair(gpu_ctx, oracle, flat, seed=3 + n, chains=2, burn=2, iters=3)
        seen += debug()
    assert any(d["copies"] > 1 for d in seen) and any(d["copies"] == 1 for d in seen)
    assert all(d["teams"] == 1 for d in seen if S == 1 or d["cache_mode"] == 1)
    if S > 1:
        assert any(d["teams"] > 1 for d in seen) and all(d["teams"] <= S for d in seen)


# --------------------------------------------------------------------------------------------------------------------------------------
# (c) table modes, each boundary from both sides, with nested groups (multicluster k-mers: NMm > 0) and single clusters in every batch
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,mode", [(6, "dense"), (7, "tagged")])
def test_dense_table_limit(gpu_ctx, oracle, debug, monkeypatch, S, mode):
    """dense_limit (bt_gibbs.hip: plan_tiles): a tile's dense tables take S x Dcm x (8 + 16 with multicluster k-mers) bytes per vertex and lane.
    64 nested groups (root H = 128: Dcm = 8 384; three vertices) in one 64-wide tile (BT_GIBBS_TAIL_WIDTH=64): 8 384 S x 24 x 64 x 3 bytes is
    231.8 MB at S = 6 (dense) and 270.4 MB at S = 7, over the 256 MB limit (the tagged direct-mapped cache)"""
    from bayestyper_amd import synth

    monkeypatch.setenv("BT_GIBBS_TAIL_WIDTH", "64")
    specs = [nested(128, kids=((2, 4), (2, 3)), flank=1) for _ in range(64)] + [single(4, kpa=2) for _ in range(8)]
    flat = synth.make_edge_batch(specs, S, seed=800 + S)
    run_pair(gpu_ctx, oracle, flat, seed=19, chains=2, burn=1, iters=2)
    big = [d for d in debug() if d["Hm"] == 128]
    assert len(big) == 1 and big[0]["lanes"] == 64 and big[0]["nvm"] == 3 and big[0]["NMm"] > 0, big
    assert big[0]["cache_mode"] == (0 if mode == "dense" else 1), big
    if mode == "tagged":
        assert big[0]["table"] == "tagged" and big[0]["teams"] == 1


def test_whole_table_rebuild_vs_invalidation(gpu_ctx, oracle, debug):
    """BT_UC_INVALIDATE_MIN = 64 (bt_gibbs_tile.hpp: cache_clear): at S = 1 a dense table of H = 9 has 54 entries (rebuilt whole when the noise
    drivers clear it), of H = 10 65 (invalidated block-wise, refilled on demand).  Single clusters and nested groups of both, and clusters of 20
    candidates (larger tables), through the noise drivers' loop, which clears the tables after every sweep.  (These tables are in HBM: the whole GPU
    invalidates them, "wide"; a table a tile invalidates itself is in test_per_sample_cache_cut[30-7].)"""
    from bayestyper_amd import synth

    S = 1
    specs = ([single(10, kpa=1, flank=2) for _ in range(16)] + [single(9, kpa=1, flank=2) for _ in range(16)] + [nested(10) for _ in range(4)] +
             [nested(9) for _ in range(4)] + [single(20, kpa=1) for _ in range(4)])
    flat = synth.make_edge_batch(specs, S, seed=810)
    luts = _oracle.build_luts(oracle, S)
    tables = [_oracle.build_luts(oracle, S, noise_rate=r)[1] for r in (0.2, 0.01, 0.1)]
    assert run_noise_loop(gpu_ctx, oracle, flat, luts, tables) > 0
    seen = debug()
    by_h = {}
    for d in seen:
        by_h.setdefault(d["Hm"], set()).add(d["table"])
    assert by_h[9] == {"whole"} and by_h[10] and by_h[10] <= {"invalidated", "wide"}, by_h
    assert {d["entries"] for d in seen if d["Hm"] == 9} == {54} and {d["entries"] for d in seen if d["Hm"] == 10} == {65}
    assert any(d["NMm"] > 0 for d in seen if d["Hm"] == 10) and any(d["NMm"] > 0 for d in seen if d["Hm"] == 9)


@pytest.mark.parametrize("S,H_on", [(30, 7), (3, 112)])
def test_per_sample_cache_cut(gpu_ctx, oracle, debug, S, H_on):
    """the per-sample cache is switched off (scache_n = 0) once 2S x min(2S, H) x (H + 1) > 4096: at S = 30 between H = 7 (3 360) and H = 8 (4 320),
    at S = 3 between H = 112 (4 068) and H = 113 (4 104).  Single clusters and nested groups on both sides; S = 30 through the noise drivers' loop"""
    from bayestyper_amd import synth

    specs = []
    n = 16 if H_on < 16 else 4
    for H in (H_on, H_on + 1):
        specs += [single(H, kpa=1, flank=1) for _ in range(n)] + [nested(H) for _ in range(4)]
    if S == 30:   # + two-haplotype clusters: a simple tile's table of 30 x 5 entries is invalidated by the tile itself when the noise counts clear it
        specs += [single(2, kpa=2) for _ in range(64)]
    flat = synth.make_edge_batch(specs, S, seed=820 + S)
    if S == 30:
        tables = [_oracle.build_luts(oracle, S, noise_rate=r)[1] for r in (0.2, 0.01)]
        run_noise_loop(gpu_ctx, oracle, flat, _oracle.build_luts(oracle, S), tables, n_it=6)
    else:
        run_pair(gpu_ctx, oracle, flat, seed=23, chains=2, burn=2, iters=2)
    seen = debug()
    on = [d for d in seen if d["Hm"] == H_on]
    off = [d for d in seen if d["Hm"] == H_on + 1]
    assert on and off
    assert all(d["scache_n"] == 2 * S * min(2 * S, H_on) for d in on), on
    assert all(d["scache_n"] == 0 for d in off), off
    assert any(d["nvm"] > 1 for d in on) and any(d["nvm"] > 1 for d in off)
    if S == 30:
        assert [(d["kernel"], d["entries"], d["table"]) for d in seen if d["Hm"] == 2] == [("simple", 150, "invalidated")]


# --------------------------------------------------------------------------------------------------------------------------------------
# (d) uchar arithmetic: the reference sums multiplicities in unsigned char (VariantClusterHaplotypes.cpp:45-108), so they wrap
# --------------------------------------------------------------------------------------------------------------------------------------
def index_luts(S):
    """a table whose every (sample, multiplicity, count) entry differs: lut_g[s][m][c] = -(1 + 1e-3 s + 1e-2 m + 1e-5 c); multiplicity 0 reads the
    noise table (values of its own), so lut_g[s][0] holds a value that a wrong read would show"""
    s, m, c = np.ogrid[:S, :256, :256]
    g = -(1 + 1e-3 * s + 1e-2 * m + 1e-5 * c)
    g[:, 0, :] = -50.0
    n = -(1.5 + 1e-3 * np.arange(S)[:, None] + 3e-5 * np.arange(256)[None, :])
    return np.ascontiguousarray(g.reshape(-1)), np.ascontiguousarray(n.reshape(-1))


def wrap_mult(H, V, kpa, flank, ic_kmers):
    """(K, H) haplotype multiplicities whose diplotype sums wrap: flank rows 128 + 128 (= 0: the noise table and the noise tally), 200 / 100
    (300 = 44, 400 = 144), 255 / 1 (256 = 0, 510 = 254); the allele rows cycle through such values; the ic rows 255 (+ ic 1 or 2)"""
    K = 2 * V * kpa + flank + ic_kmers
    vals = np.array([128, 200, 100, 255, 1, 130, 127, 64])
    k, h = np.ogrid[:K, :H]
    M = vals[(3 * k + h) % len(vals)]
    fl = 2 * V * kpa
    M[fl] = 128
    M[fl + 1] = np.where(np.arange(H) % 2 == 0, 200, 100)
    M[fl + 2] = np.where(np.arange(H) % 2 == 0, 255, 1)
    M[K - ic_kmers:K] = 255
    return M


def uchar_batch(S, seed, nested_groups=True):
    """two-haplotype clusters (gibbs_simple_kernel: a 64-wide tile of their own), clusters of 5..10 candidates (gibbs_hot_kernel) and nested groups whose multicluster sums
    wrap (shared - dip(prev) + dip(new) + ic: 60 per haplotype on both sides of the shared k-mers, ic 30; the shared total itself stays <= 240,
    as the reference asserts), with counts 0 and 255 written over some rows"""
    from bayestyper_amd import synth

    specs, counts = [], {}
    for _ in range(64):
        specs.append(single(2, kpa=2, flank=3, ic_kmers=2, ic=(1, 2), mult=wrap_mult(2, 1, 2, 3, 2)))
    for H in (5,) * 64 + (6, 7, 8, 9, 10) * 3:
        specs.append(single(H, kpa=1, flank=3, ic_kmers=2, ic=(1, 2), mult=wrap_mult(H, V_of(H), 1, 3, 2)))
    for _ in range(4 if nested_groups else 0):
        specs.append(nested(8, kids=((2, 4),), flank=3, mult=wrap_mult(8, 3, 1, 3, 0), shared_mult=(60, 60), shared_ic=(30, 30)))
    for g, spec in enumerate(specs):
        fl = 2 * spec["V"] * spec.get("kpa", 1)
        counts[(g, 0, fl)] = [0, 255, 17]
        counts[(g, 0, fl + 1)] = 255
        counts[(g, 0, fl + 2)] = 0
        if "kids" in spec:   # the root's shared k-mer (after its flank rows): unobserved in sample 0 (dip + ic), saturated in sample 1
            counts[(g, 0, fl + 3)] = [0, 255, 40]
    return synth.make_edge_batch(specs, S, seed, gender=[0, 1, 0], counts=counts)


def test_uchar_multiplicity_wrap(gpu_ctx, oracle, debug, monkeypatch):
    """wrapped multiplicities read the table at [s][m mod 256][c] — multiplicity 0 the noise table — in the two-haplotype kernel, the hot kernel,
    the multicluster sums of nested groups and the noise tally, with a table where a wrong index changes the log-probability.
    Regression: an allele k-mer mean over a count divided by a wrapped multiplicity of 0 is infinite; the reference's next Welford step turns it
    into NaN (inf - inf), while the repeated-value shortcut of the collected statistics (bt_gibbs_tile.hpp: ks_add_rep) kept it infinite"""
    S = 3
    flat = uchar_batch(S, seed=840)
    M = flat["hap_kmer_mult"]
    assert (M == 128).any() and (M == 255).any() and (flat["kmer_counts"] == 0).any() and (flat["kmer_counts"] == 255).any()
    kw = dict(seed=41, chains=3, burn=5, iters=10)
    luts = index_luts(S)
    base = run_pair(gpu_ctx, oracle, flat, luts=luts, **kw)
    seen = debug()
    # (the nested groups keep every vertex's hot arrays in LDS, so gibbs_hot_kernel runs their multicluster sums too; gibbs_kernel gets them
    # under BT_GIBBS_NO_HOT_KERNEL in check_kernel_paths)
    assert {"simple", "hot"} <= {d["kernel"] for d in seen}, seen
    assert any(d["NMm"] > 0 and d["nvm"] > 1 for d in seen), seen
    check_kernel_paths(gpu_ctx, flat, luts, base, monkeypatch, debug, **kw)
    # the noise-seeded sampler: k-mers whose multiplicity wraps to 0 are tallied as noise.  (Single clusters only: the noise tally counts unique
    # k-mers, and reset_groups keeps the shared multiplicities — as VariantClusterGroup::resetGroup does —, so over two chains the nested groups'
    # 60-per-haplotype shared k-mers would sum past 255, where the reference asserts (updateMulticlusterKmerMultiplicities: pre <= m).)
    flat = uchar_batch(S, seed=841, nested_groups=False)
    n = luts[1]
    tables = [n - 0.25, n - 0.5 - 1e-4 * np.tile(np.arange(256), S)]
    assert run_noise_loop(gpu_ctx, oracle, flat, luts, tables) > 0


# --------------------------------------------------------------------------------------------------------------------------------------
# (e) the draw path: linear-domain draws verified against a margin, the logAddition chain inside it
# --------------------------------------------------------------------------------------------------------------------------------------
def draw_luts(S, kind):
    s, m, c = np.ogrid[:S, :256, :256]
    cn = np.arange(256)[None, :]
    sn = np.arange(S)[:, None]
    if kind == "amplified":   # |entry| ~ 1e9 with O(1) differences
        g = -(1e9 + 1 + 0.25 * np.abs(c / 15.0 - m) + 1e-3 * s)
        n = -(1e9 + 1.5 + 0.25 * cn / 15.0 + 1e-3 * sn)
    elif kind == "flat":      # candidates differ only through their frequency terms
        g = np.full((S, 256, 256), -2.5)
        n = np.full((S, 256), -2.5)
    else:                     # steep: one multiplicity step costs 350, exp(lp - lpmax) is subnormal or zero for most candidates
        g = -(1 + 350 * np.abs(c / 15.0 - m) + 1e-3 * s)
        n = -(1 + 350 * cn / 15.0 + 1e-3 * sn)
    g = np.broadcast_to(g, (S, 256, 256))
    n = np.broadcast_to(n, (S, 256))
    assert np.isfinite(g).all() and np.isfinite(n).all()
    return np.ascontiguousarray(g.reshape(-1), np.float64), np.ascontiguousarray(n.reshape(-1), np.float64)


@pytest.mark.parametrize("kind", ["amplified", "flat", "steep"])
def test_draw_path_margin_fallback(gpu_ctx, oracle, debug, monkeypatch, kind):
    """64 clusters of H = 8 (V = 3, 14 k-mers: gibbs_hot_kernel) and 64 of H = 2 (14 k-mers: gibbs_simple_kernel), S = 3, 4 chains x 60 sweeps, every
    k-mer in the subset (rate 1): 46 080 diplotype draws per class.

    "amplified": every table entry is -1e9 - O(1), so a candidate's log-probability sums 14 of them: |lp| >= 1.4e10.  A draw over T > 4 candidates
    (bt_gibbs_tile.hpp: sample_diplotypes) is taken in the linear domain and kept only when U x total lies farther than
        margin = max(64 T |lpmax| eps, 1e-6) x total >= 64 x 5 x 1.4e10 x 2.2e-16 x total ~ 1e-3 x total
    from both ends of the picked interval; otherwise the reference's logAddition chain decides.  The band below the grand total alone is 1e-3 of
    U's range, so at least one such draw in a thousand takes the chain, and with the bands of the T - 1 inner boundaries (2 x margin each, T up to
    36) a few percent do: thousands of chain decisions in the run, where the suite's tables (|lp| ~ 10..10^4) give one in 10^5..10^6.  The
    two-haplotype kernel's own check (bt_gibbs_simple.hpp: U x total within 1e-5 x total of a boundary) sees log-probabilities whose ulp is 2e-6.
    A rounding or summation-order difference against the reference would flip decisions at a rate near 1e-3 here: the traces must stay equal.
    "flat": every entry -2.5, candidates differ only through their frequency terms (near-ties); "steep": a multiplicity step costs 350, so
    exp(lp - lpmax) is subnormal or zero for most candidates.  All entries are finite (logAddition(-inf, -inf) is NaN in the reference)."""
    from bayestyper_amd import synth

    S = 3
    specs = [single(8, kpa=2, flank=2) for _ in range(64)] + [single(2, kpa=6, flank=2) for _ in range(64)]
    flat = synth.make_edge_batch(specs, S, seed=850)
    assert set(np.diff(flat["kmer_off"]).tolist()) == {14}
    kw = dict(seed=61, chains=4, burn=20, iters=40, rate=1.0)
    luts = draw_luts(S, kind)
    base = run_pair(gpu_ctx, oracle, flat, luts=luts, **kw)
    hm = {}
    for d in debug():
        hm.setdefault(d["kernel"], set()).add(d["Hm"])
    assert hm.get("simple") == {2} and hm.get("hot") == {8}, hm
    if kind == "amplified":
        check_kernel_paths(gpu_ctx, flat, luts, base, monkeypatch, debug, **kw)


# --------------------------------------------------------------------------------------------------------------------------------------
# (g) ploidy 0, 1 and 2 within a group at S = 30
# --------------------------------------------------------------------------------------------------------------------------------------
def test_mixed_ploidy_thirty_samples(gpu_ctx, oracle, debug):
    """ploidy 0 / 1 / 2 mixed within every group, a group where every sample has ploidy 0, male samples (gender 1: the male intercluster
    multiplicities) haploid on X-like groups, across two-haplotype, multi-candidate and nested groups"""
    from bayestyper_amd import synth

    S = 30
    specs = ([single(2, kpa=2, ic_kmers=1, ic=(1, 2)) for _ in range(64)] + [single(7, kpa=1, ic_kmers=2, ic=(1, 2)) for _ in range(8)] +
             [single(10, kpa=1, flank=2) for _ in range(4)] + [nested(8) for _ in range(4)])
    G = len(specs)
    rng = np.random.default_rng(860)
    gender = np.arange(S) % 2
    ploidy = rng.choice(np.array([0, 1, 2], np.uint8), size=(G, S), p=[0.15, 0.25, 0.6])
    ploidy[::3, gender == 1] = 1    # X-like: males haploid
    ploidy[1::3, gender == 0] = 0   # Y-like: absent in females
    ploidy[G - 1] = 0
    flat = synth.make_edge_batch(specs, S, seed=861, ploidy=ploidy, gender=gender)
    for g in range(G):
        assert g == G - 1 or len(set(ploidy[g].tolist())) >= 2, g
    run_pair(gpu_ctx, oracle, flat, seed=71, chains=2, burn=3, iters=5)
    assert {"simple", "hot"} <= {d["kernel"] for d in debug()}


def test_one_haplotype_candidate(gpu_ctx, oracle, debug):
    """H = 1: bt_gibbs_create accepts a cluster with a single haplotype candidate (the only diplotype is (0, 0)); it samples as the oracle does"""
    from bayestyper_amd import synth

    # (the reference's sparsity estimate asserts that every k-mer is on some candidate: the cluster has no alternative-allele k-mers)
    flat = synth.make_edge_batch([dict(V=1, H=1, kpa=[[2, 0]], flank=1) for _ in range(8)], 3, seed=911)
    run_pair(gpu_ctx, oracle, flat, seed=3, chains=2, burn=2, iters=3)
    assert {d["Hm"] for d in debug()} == {1}
