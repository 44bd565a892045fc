"""bt_gibbs_genotype_text / bt_genotype_text: the genotype text of a launch formatted on the device against the same header code run on the host
(bt_diag_genotype_text over the records Gibbs.genotypes returns from the same sampler: bytes and words) and against the host layer's stream formatters
(byte for byte).  Every sampler runs 3 chains x (10 + 40) sweeps.  Then hand-built record strings (_genotype_text.py) through bt_genotype_text against a reference
made of Python's '%g' alone and against bt_diag_genotype_text: the offsets scan past one workgroup, format_g6 at its edges, StoreSink at every alignment."""
import ctypes as C

import numpy as np
import pytest

import _oracle
from _genotype_text import (SCAN_BLOCK, SCAN_CASES, alignment_case, assert_launch_text_equals_host, check_against_reference, check_alignment_inputs, check_g6_inputs,
                            check_scan_inputs, g6_case, hand_written, make_string, not_covered_case, ploidy_word, scan_case)
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


# ---- hand-built strings: each has a twin in test_genotype_text_cpu.py that checks the input's conditions and the reference without a GPU ----------------------
GUARD = 64


def _device_against_reference_and_host(gpu_ctx, words, ref, what, shift=0):
    """bt_genotype_text with the text at a 4-aligned address + shift, its capacity the exact size, GUARD bytes of 0xAA on both sides: the text, the index, the
    sizes and the count are the reference's and bt_diag_genotype_text's, and no byte outside the text changed.  -> (index, address of the text)"""
    from bayestyper_amd import lib

    h_text, h_index, h_nc = lib.diag_genotype_text(words)
    d = gpu_ctx.to_device(words)
    n = ref.text.size
    assert lib.genotype_text_sizes(gpu_ctx, d.ptr, words.size) == (n, ref.index.size), what
    d_buf, d_index = gpu_ctx.to_device(np.full(n + 2 * GUARD + 8, 0xAA, np.uint8)), gpu_ctx.to_device(np.full(ref.index.size, 0xAAAAAAAA, np.uint32))
    start = (-d_buf.ptr) % 4 + GUARD + shift
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    lib.check(lib.bt_genotype_text(gpu_ctx.h, d.ptr, words.size, d_buf.ptr + start, n, d_index.ptr, ref.index.size, C.byref(nt), C.byref(ni), C.byref(nc)))
    buf, index = d_buf.download(np.uint8, n + 2 * GUARD + 8), d_index.download(np.uint32, ref.index.size)
    address = d_buf.ptr + start
    for b in (d, d_buf, d_index):
        b.free()
    assert (nt.value, ni.value) == (n, ref.index.size), what
    text = buf[start:start + n]
    check_against_reference(text, index, nc.value, ref, what)
    assert nc.value == h_nc and np.array_equal(index, h_index) and np.array_equal(text, h_text), what
    assert (buf[:start] == 0xAA).all() and (buf[start + n:] == 0xAA).all(), (what, "bytes outside the text were written")
    return index, address


@pytest.mark.parametrize("NV,S,multi", SCAN_CASES)
def test_scan_past_one_workgroup(gpu_ctx, NV, S, multi):
    """text_scan_block_kernel / text_scan_add_kernel with one to five workgroups, NV = 1, 2, 3 mod 4, NV = 0, S = 0, C != NV; from 2049 variants on with
    not-covered variants in every scan block"""
    from bayestyper_amd import lib

    words, ref, variants = scan_case(NV, S, multi)
    check_scan_inputs(NV, S, multi, ref, variants)
    index, _ = _device_against_reference_and_host(gpu_ctx, words, ref, f"NV={NV} S={S} multi={multi}")
    if NV > SCAN_BLOCK:   # (check_against_reference has compared every offset; this names the scan)
        at = 5 + ref.Cn + 9 * SCAN_BLOCK
        assert int(index[at]) | (int(index[at + 1]) << 32) == ref.variant_offset(SCAN_BLOCK), "the offset of the second scan block's first variant"
    assert index[5 + ref.Cn + 8:5 + ref.Cn + 9 * NV:9].tolist() == ref.flags.tolist()
    d = gpu_ctx.to_device(words)   # the wrapper that sizes its own buffers
    text, index2, not_covered = lib.genotype_text(gpu_ctx, d.ptr, words.size)
    d.free()
    check_against_reference(text, index2, not_covered, ref, "lib.genotype_text")


def test_a_malformed_record_past_the_first_scan_block_writes_nothing(gpu_ctx):
    from bayestyper_amd import lib

    words, ref, _ = scan_case(2049, 1)
    bad = words.copy()
    bad[ploidy_word(words, 1500)] = 3
    d, d_text, d_index = gpu_ctx.to_device(bad), gpu_ctx.to_device(np.full(ref.text.size, 0xAA, np.uint8)), gpu_ctx.to_device(np.full(ref.index.size, 0xAAAAAAAA, np.uint32))
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert lib.bt_genotype_text(gpu_ctx.h, d.ptr, bad.size, d_text.ptr, ref.text.size, d_index.ptr, ref.index.size, C.byref(nt), C.byref(ni), C.byref(nc)) != 0
    assert "layout" in lib.bt_last_error().decode()
    assert (d_text.download(np.uint8, ref.text.size) == 0xAA).all() and (d_index.download(np.uint32, ref.index.size) == 0xAAAAAAAA).all()
    for b in (d, d_text, d_index):
        b.free()


def test_format_g6_edges_on_the_device(gpu_ctx):
    """the device's digits against Python's '%g': ties, both notation switches, negative values, doubles that are no widened floats, 5 - floor(log10 v) >= 27"""
    check_g6_inputs()
    words, ref = g6_case()
    assert ref.not_covered == 0
    _device_against_reference_and_host(gpu_ctx, words, ref, "format_g6 values")


def test_not_covered_values_on_the_device(gpu_ctx):
    """NaN, the infinities, subnormals, 1e6 and what lies below 1e-27, each in a variant of its own: flagged and counted, nothing printed for the value, the
    variants between them untouched"""
    words, ref, at = not_covered_case()
    assert ref.not_covered == len(at) > 10
    index, _ = _device_against_reference_and_host(gpu_ctx, words, ref, "not covered")
    assert np.flatnonzero(index[5 + ref.Cn + 8:5 + ref.Cn + 9 * ref.NV:9]).tolist() == at


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_store_alignment(gpu_ctx, shift):
    """StoreSink's whole-dword and byte stores: every (first byte, one past the last byte) residue among the cells, the variant pieces and the seams between
    the two write kernels, the text buffer at a 4-aligned address + shift, guard bytes on both sides"""
    words, ref, variants = alignment_case()
    for a in range(4):   # (a condition on the lengths: it holds at every address)
        check_alignment_inputs(ref, variants, a)
    _, address = _device_against_reference_and_host(gpu_ctx, words, ref, f"shift {shift}", shift)
    assert address % 4 == shift
    check_alignment_inputs(ref, variants, address)
