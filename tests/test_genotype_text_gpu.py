"""bt_gibbs_genotype_text / bt_genotype_text: the genotype text of a launch formatted on the device against the same header code run on the host
(bt_diag_genotype_text over the records Gibbs.genotypes returns from the same sampler: bytes and words) and against the host layer's stream formatters
(byte for byte).  Every sampler runs 3 chains x (10 + 40) sweeps."""
import ctypes as C

import numpy as np
import pytest

import _oracle
from _genotype_text import assert_launch_text_equals_host, hand_written, make_string
from _genotypes_device import group_of_cluster, min_fraction, mixed_batch, multiallelic_batch
from test_genotype_text_cpu import check_hand_written
from test_genotypes_device_gpu import same_results

pytestmark = pytest.mark.gpu

KW = dict(seed=11, chains=3, burn=10, iters=40)
MIN_GPP, MIN_KMERS = 0.99, 1.0


def _sampler(gpu_ctx, oracle, flat, S):
    from bayestyper_amd import lib

    g = lib.Gibbs(gpu_ctx, flat, *_oracle.build_luts(oracle, S), **KW)
    g.run()
    return g


def _check_launch(g, flat, ploidy, S, what):
    from bayestyper_amd import lib

    mf = min_fraction(S)
    before = g.results()
    text, index, not_covered = g.genotype_text(MIN_GPP, MIN_KMERS, mf)
    after = g.results()
    assert same_results(before, after), what   # the sampler's state is untouched
    words = g.genotypes(MIN_GPP, MIN_KMERS, mf)   # ... and genotypes still works afterwards
    h_text, h_index, h_not_covered = lib.diag_genotype_text(words)
    assert not_covered == h_not_covered == 0
    assert np.array_equal(index, h_index) and np.array_equal(text, h_text), what
    NV = int(np.sum(flat["num_variants"]))
    assert (int(index[0]), int(index[1]), int(index[2])) == (flat["num_clusters"], NV, S) and text.size > 20 * NV * S
    group = group_of_cluster(flat)
    assert_launch_text_equals_host(lib.parse_genotype_text(text, index), flat, after, [ploidy[group[c]] for c in range(flat["num_clusters"])], mf, what=what)
    # a second call returns the same, and so does the entry over the record string where bt_gibbs_genotypes left it
    text2, index2, _ = g.genotype_text(MIN_GPP, MIN_KMERS, mf)
    assert np.array_equal(text, text2) and np.array_equal(index, index2)
    return words


@pytest.mark.parametrize("S", [3, 10])
def test_mixed_batch(gpu_ctx, oracle, S):
    """S = 10: the cell-to-lane mapping when S does not divide 64"""
    flat, ploidy = mixed_batch(S)
    g = _sampler(gpu_ctx, oracle, flat, S)
    _check_launch(g, flat, ploidy, S, f"mixed S={S}")
    g.close()


def test_multiallelic_batch_wider_than_a_wavefront(gpu_ctx, oracle):
    """78 groups: more than one wavefront of cells, tiles wider than 64 groups, A = 2 .. 7"""
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = multiallelic_batch(S, n_small=70)
    assert int(np.sum(flat["num_variants"])) * S > 256
    g = _sampler(gpu_ctx, oracle, flat, S)
    words = _check_launch(g, flat, ploidy, S, "multiallelic")
    # the entry over any record string in device memory, with the caller's buffers: the same text and index
    d = gpu_ctx.to_device(words)
    h_text, h_index, _ = lib.diag_genotype_text(words)
    assert lib.genotype_text_sizes(gpu_ctx, d.ptr, words.size) == (h_text.size, h_index.size)
    text, index, not_covered = lib.genotype_text(gpu_ctx, d.ptr, words.size)
    assert not_covered == 0 and np.array_equal(text, h_text) and np.array_equal(index, h_index)
    d.free()
    g.close()


def test_hand_written_string_on_the_device(gpu_ctx):
    """the CPU test's string with a 1e7 mean and a NaN posterior: the same flags, count and text as the host diagnostic; a small capacity writes nothing"""
    from bayestyper_amd import lib

    S = 2
    variants = hand_written(S)
    words = make_string(S, variants)
    h_text, h_index, h_nc = lib.diag_genotype_text(words)
    d = gpu_ctx.to_device(words)
    text, index, not_covered = lib.genotype_text(gpu_ctx, d.ptr, words.size)
    assert not_covered == h_nc == 2 and np.array_equal(text, h_text) and np.array_equal(index, h_index)
    check_hand_written(text, index, not_covered, variants, S)
    d_text, d_index = gpu_ctx.to_device(np.full(h_text.size, 0xAA, np.uint8)), gpu_ctx.to_device(np.full(h_index.size, 0xAAAAAAAA, np.uint32))
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    for tcap, icap in ((h_text.size - 1, h_index.size), (h_text.size, h_index.size - 1)):
        assert lib.bt_genotype_text(gpu_ctx.h, d.ptr, words.size, d_text.ptr, tcap, d_index.ptr, icap, C.byref(nt), C.byref(ni), C.byref(nc)) != 0
        assert "bt_genotype_text: buffer too small" in lib.bt_last_error().decode() and (nt.value, ni.value) == (h_text.size, h_index.size)
        assert (d_text.download(np.uint8, h_text.size) == 0xAA).all() and (d_index.download(np.uint32, h_index.size) == 0xAAAAAAAA).all()
    assert lib.bt_genotype_text(gpu_ctx.h, None, words.size, d_text.ptr, h_text.size, d_index.ptr, h_index.size, C.byref(nt), C.byref(ni), C.byref(nc)) != 0
    assert "bt_genotype_text: null argument" in lib.bt_last_error().decode()
    bad = words.copy()
    bad[int(words[5 + 5]) + 4 + 4 * 2] = 3   # ploidy 3 in the first sample record: refused before anything is written
    db = gpu_ctx.to_device(bad)
    assert lib.bt_genotype_text(gpu_ctx.h, db.ptr, bad.size, d_text.ptr, h_text.size, d_index.ptr, h_index.size, C.byref(nt), C.byref(ni), C.byref(nc)) != 0
    assert "layout" in lib.bt_last_error().decode() and (d_text.download(np.uint8, h_text.size) == 0xAA).all()
    for b in (d, db, d_text, d_index):
        b.free()


def test_errors(gpu_ctx, oracle):
    from bayestyper_amd import lib

    S = 3
    flat, ploidy = mixed_batch(S)
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    g = lib.Gibbs(gpu_ctx, flat, lut_g, lut_n, **KW)
    with pytest.raises(lib.BtError, match="bt_gibbs_genotype_text: nothing was collected yet"):
        g.genotype_text(MIN_GPP, MIN_KMERS, min_fraction(S))
    pt, pi, nt, ni, nc = lib.vp(), lib.vp(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    f, keep = lib._genotype_filters(MIN_GPP, MIN_KMERS, min_fraction(S))
    full = [g.h, C.addressof(f), C.byref(pt), C.byref(nt), C.byref(pi), C.byref(ni), C.byref(nc)]
    for i in range(len(full)):
        args = list(full)
        args[i] = None
        assert lib.bt_gibbs_genotype_text(*args) != 0 and "bt_gibbs_genotype_text: null argument" in lib.bt_last_error().decode()
    g.close()
    g = lib.Gibbs(gpu_ctx, flat, lut_g, lut_n, seed=5, chains=1, burn=1, iters=4, noise_seeding=1)
    g.set_noise_lut(lut_n)
    g.init_chain(0)
    assert g.noise_chain_begin(5, 1)
    for _ in range(2):   # (the resident launch is in flight from the second step on at the latest)
        g.noise_chain_step(None)
    with pytest.raises(lib.BtError, match=r"bt_gibbs_genotype_text: a resident noise chain is in progress \(bt_gibbs_noise_chain_end\)"):
        g.genotype_text(MIN_GPP, MIN_KMERS, min_fraction(S))
    for _ in range(3):   # the chain still ends normally, and the text of what it collected is the host's
        g.noise_chain_step(None)
    g.noise_chain_end()
    _check_launch(g, flat, ploidy, S, "after the chain")
    g.close()
