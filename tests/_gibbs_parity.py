"""Parity helpers of the Gibbs GPU tests (tests/test_gibbs_gpu.py, tests/test_gibbs_edges_gpu.py): the GPU sampler and the oracle on the same
batch, seed and tables; diplotype posteriors and allele k-mer statistics compared."""
import numpy as np

import _oracle

TOL = 1e-4   # posterior tolerance stated by north_star


def run_both(gpu_ctx, oracle, flat, trace=0, flat_gpu=None, **kw):
    """the oracle on `flat`, the GPU on `flat_gpu` (default: the same batch)"""
    from bayestyper_amd import lib

    S = flat["S"]
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    og = _oracle.OrcGibbs(oracle, flat, lut_g, lut_n, **kw)
    gg = lib.Gibbs(gpu_ctx, flat if flat_gpu is None else flat_gpu, lut_g, lut_n, **kw)
    if trace:
        og.trace_enable(trace)
        gg.trace_enable(trace)
    og.run(8)
    gg.run()
    gpu_ctx.sync()
    ro, rg = og.results(), gg.results()
    # the same results as the word string a rank hands to the gather (bt_gibbs_result_words, packed on the device)
    rw, used = lib.parse_result_words(gg.result_words_host())
    assert used == gg.result_words()[1] and set(rw) == set(rg)
    for key in rg:
        assert np.array_equal(rw[key], rg[key], equal_nan=(key == "stats")), key
    tr = None
    if trace:
        goff = flat["group_cluster_off"]
        tg = gg.trace()
        tr = [(og.trace(g, int(goff[g + 1] - goff[g]), trace), tg[g]) for g in range(flat["num_groups"])]
    og.close()
    gg.close()
    return ro, rg, tr


def posteriors(r, c, S):
    """{(h1,h2): freq/total} per sample for cluster c"""
    e0, e1 = int(r["dip_off"][c]), int(r["dip_off"][c + 1])
    tot = r["freq"][e0:e1].sum(axis=0).astype(np.float64)
    return {(int(r["h1"][e]), int(r["h2"][e])): r["freq"][e] / np.maximum(tot, 1) for e in range(e0, e1)}, tot


def assert_parity(flat, ro, rg, n_collect):
    S = flat["S"]
    exact = 0
    for c in range(flat["num_clusters"]):
        po, to = posteriors(ro, c, S)
        pg, tg = posteriors(rg, c, S)
        assert (to == n_collect).all() and (tg == n_collect).all()
        keys = set(po) | set(pg)
        worst = max(np.abs(po.get(k, np.zeros(S)) - pg.get(k, np.zeros(S))).max() for k in keys)
        assert worst <= TOL, f"cluster {c}: diplotype posterior differs by {worst}"
        exact += int(worst == 0)
    # allele k-mer statistics (NAK/FAK/MAC inputs): counts exact, means to 1e-9 relative
    so, sg = ro["stats"], rg["stats"]
    assert so.shape == sg.shape
    assert np.array_equal(so[:, :, 0], sg[:, :, 0])
    assert np.allclose(so[:, :, 1:3], sg[:, :, 1:3], rtol=1e-9, atol=1e-12)
    return exact
