"""The genotype text of the device route without a GPU: bt_diag_format_g6 and bt_diag_genotype_text run the __host__ __device__ code of the text kernels
(bayestyper_amd/csrc/bt_genotype_text.hpp) on the host.  The number formatter against Python's '%g' (correctly rounded, as glibc's printf), the three pieces of
every variant against the host layer's stream formatters, byte for byte.  All of it fails without the text entries."""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle
from _genotype_text import (G6_RANGE_EDGES, SCAN_BLOCK, SCAN_CASES, alignment_case, assert_cluster_text_equals_host, check_against_reference, check_alignment_inputs,
                            check_g6_inputs, check_scan_inputs, expected_pieces, g6_case, g6_doubles, g6_floats, g6_near_switches, g6_not_covered, g6_ties, hand_written,
                            make_string, not_covered_case, ploidy_word, scan_case)
from _genotypes_device import group_of_cluster, min_fraction, mixed_batch, multiallelic_batch
from bayestyper_amd import lib


def _check_g6(values, what, allow_not_covered=False):
    values = np.ascontiguousarray(values, np.float64)
    got = lib.diag_format_g6(values)
    bad = [(float(v), g, "%g" % v) for v, g in zip(values, got) if g != "%g" % v and not (allow_not_covered and g is None)]
    assert not bad, (what, len(bad), bad[:10])
    return got


def test_float32_ratios():
    """every float32 k / N for N in 1 .. 64 and N in {250, 5000, 7000} (posteriors are multiples of 1 / sweeps), widened to double as the host's operator<< does"""
    for N in list(range(1, 65)) + [250, 5000, 7000]:
        k = np.arange(N + 1, dtype=np.float32)
        _check_g6((k / np.float32(N)).astype(np.float64), f"k/{N}")


def test_double_ratios():
    """a / b for a < 10^5, b <= 10^3 (k-mer means): a stride of a keeps the test quick, every b and every residue of a mod 10 is met"""
    b = np.arange(1, 1001, dtype=np.float64)
    for a0 in range(0, 100000, 9973):
        a = np.arange(a0, min(a0 + 137, 100000), dtype=np.float64)
        _check_g6((a[:, None] / b[None, :]).reshape(-1), f"a/b from a = {a0}")
    a = np.arange(0, 100000, 7, dtype=np.float64)
    _check_g6((a[:, None] / np.array([1, 2, 3, 7, 10, 16, 64, 125, 999, 1000], np.float64)[None, :]).reshape(-1), "a/b over all a")


def test_exact_ties_round_to_even():
    """(D + 0.5) / 10^p whose quotient is exactly representable: the seventh digit is an exact 5, and %g rounds the sixth to even"""
    ties = g6_ties()
    assert len(ties) > 1000   # (p = 0 always; p >= 1 when (2 D + 1) / 2 is a multiple of 5^p)
    assert sum(1 for v in ties if v != math.floor(v) + 0.5) > 10
    _check_g6(ties, "ties")
    # near both notation switches: 10^-5 | 10^-4 (exponent / fixed) and 10^5 | 10^6 (fixed / exponent)
    near = g6_near_switches()
    got = _check_g6(near, "switches")
    assert got[near.index(999999 + 0.5)] == "1e+06" and got[5].endswith("e-05") and got[6].startswith("0.0001") and got[near.index(99999.5)] == "99999.5"


def test_range_edges():
    edges = list(G6_RANGE_EDGES)
    got = _check_g6(edges, "edges")
    assert got[:6] == ["9.99999e-05", "0.0001", "0.0001", "999999", "1e+06", "1e-27"] and got[6:9] == ["-1", "0", "-0"]
    assert lib.diag_format_g6([np.nextafter(1e-27, 0)]) == [None]


def test_not_covered_values_give_no_text():
    vals = np.array([np.inf, -np.inf, np.nan, 5e-324, 2.2250738585072009e-308, 1e6, 1e7, -1e6, 1e-28, 1e-30, np.nextafter(1e-27, 0)], np.float64)
    text, lens = np.full(vals.size * 16, 0xAA, np.uint8), np.zeros(vals.size, np.int32)
    lib.check(lib.bt_diag_format_g6(vals.ctypes.data, vals.size, text.ctypes.data, lens.ctypes.data))
    assert (lens == -1).all() and not text.any()
    assert lib.bt_diag_format_g6(None, 1, text.ctypes.data, lens.ctypes.data) != 0 and "bt_diag_format_g6: null argument" in lib.bt_last_error().decode()


def _batch_text_against_host(oracle, flat, ploidy, mf, what):
    S = flat["S"]
    lut_g, lut_n = _oracle.build_luts(oracle, S)
    og = _oracle.OrcGibbs(oracle, flat, lut_g, lut_n, seed=11, chains=3, burn=10, iters=40)
    og.run(4)
    res = og.results()
    og.close()
    group = group_of_cluster(flat)
    slots = ploidy0 = 0
    for c in range(flat["num_clusters"]):
        H, V = int(flat["num_haplotypes"][c]), int(flat["num_variants"][c])
        hv0 = int(np.sum(flat["num_haplotypes"][:c].astype(np.int64) * flat["num_variants"][:c].astype(np.int64)))
        v0 = int(np.sum(flat["num_variants"][:c]))
        e0, e1 = int(res["dip_off"][c]), int(res["dip_off"][c + 1])
        w = lib.diag_genotype_cluster(S, H, V, flat["hap_allele"][hv0:hv0 + H * V], flat["var_num_alleles"][v0:v0 + V], flat["var_has_dependency"][v0:v0 + V], res["h1"][e0:e1],
                                      res["h2"][e0:e1], res["freq"][e0:e1], res["stats"][int(res["cell_off"][c]):int(res["cell_off"][c + 1])], ploidy[group[c]], 0.99, 1.0, mf)
        text, index, not_covered = lib.diag_genotype_text(w)
        assert not_covered == 0 and (int(index[0]), int(index[1]), int(index[2]), int(index[3])) == (1, V, S, 0)
        var = index[6:6 + 9 * V].reshape(V, 9).astype(np.int64)
        # the text is contiguous in variant order and exactly sized
        assert np.array_equal(var[:, 0], np.concatenate([[0], np.cumsum(var[:, 2:5].sum(axis=1))])[:-1]) and not var[:, 1].any() and int(var[:, 2:5].sum()) == text.size
        cells = index[6 + 9 * V:].reshape(V, S, 2)
        slots += int((cells[:, :, 1] != 0xFFFFFFFF).sum())
        ploidy0 += int((cells[:, :, 1] == 0xFFFFFFFF).sum())
        assert_cluster_text_equals_host(lib.parse_genotype_text(text, index), flat, res, c, ploidy[group[c]], mf, what=what)
    return slots, ploidy0


@pytest.mark.parametrize("S", [3, 1])
def test_oracle_samples_of_the_mixed_batch(oracle, S):
    flat, ploidy = mixed_batch(S)
    slots, ploidy0 = _batch_text_against_host(oracle, flat, ploidy, min_fraction(S), f"mixed batch S={S}")
    assert slots > 10 and (ploidy0 > 0 or S == 1)


@pytest.mark.parametrize("S", [3, 1])
def test_oracle_samples_of_a_multiallelic_batch(oracle, S):
    flat, ploidy = multiallelic_batch(S, 4)
    assert set(range(2, 8)) <= set(int(a) for a in flat["var_num_alleles"])
    slots, ploidy0 = _batch_text_against_host(oracle, flat, ploidy, min_fraction(S), f"multi-allelic batch S={S}")
    assert slots > 10 and ploidy0 > 0


def check_hand_written(text, index, not_covered, variants, S):
    """the two variants with a value outside the formatter's range are flagged and counted; the others carry the text Python's '%g' gives"""
    assert not_covered == 2 and int(index[3]) == 2
    parsed = lib.parse_genotype_text(text, index)
    assert [p["flags"] for p in parsed] == [0, 1, 0, 1, 0]
    for v in (0, 2, 4):
        assert (parsed[v]["stats"], parsed[v]["cover"], parsed[v]["samples"]) == expected_pieces(variants[v]), v
        assert parsed[v]["A"] == len(variants[v]["alleles"]) and parsed[v]["total_count"] == variants[v]["total_count"]
    assert parsed[2]["cover"] == ";ANC=0,2" and parsed[2]["samples"].startswith("\t:.:.:.:.:.:.\t./.:")


def test_hand_written_string_with_not_covered_values():
    S = 2
    variants = hand_written(S)
    text, index, not_covered = lib.diag_genotype_text(make_string(S, variants))
    check_hand_written(text, index, not_covered, variants, S)


def test_small_capacity_is_an_error_and_writes_nothing():
    w = make_string(2, hand_written(2))
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert lib.bt_diag_genotype_text(w.ctypes.data, w.size, None, 0, None, 0, C.byref(nt), C.byref(ni), C.byref(nc)) != 0
    assert "bt_diag_genotype_text: buffer too small" in lib.bt_last_error().decode() and nt.value > 100 and ni.value == 4 + 6 + 5 * 9 + 5 * 2 * 2
    text, index = np.full(nt.value, 0xAA, np.uint8), np.full(ni.value, 0xAAAAAAAA, np.uint32)
    for tcap, icap in ((nt.value - 1, ni.value), (nt.value, ni.value - 1)):
        assert lib.bt_diag_genotype_text(w.ctypes.data, w.size, text.ctypes.data, tcap, index.ctypes.data, icap, C.byref(nt), C.byref(ni), C.byref(nc)) != 0
        assert "buffer too small" in lib.bt_last_error().decode() and (text == 0xAA).all() and (index == 0xAAAAAAAA).all()
    lib.check(lib.bt_diag_genotype_text(w.ctypes.data, w.size, text.ctypes.data, nt.value, index.ctypes.data, ni.value, C.byref(nt), C.byref(ni), C.byref(nc)))
    assert not (text == 0xAA).all()


def test_strings_of_another_layout_are_refused():
    w = make_string(2, hand_written(2))
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    args = (None, 0, None, 0, C.byref(nt), C.byref(ni), C.byref(nc))
    assert lib.bt_diag_genotype_text(None, 0, *args) != 0 and "null argument" in lib.bt_last_error().decode()
    assert lib.bt_diag_genotype_text(w.ctypes.data, 3, *args) != 0 and "shorter than its head" in lib.bt_last_error().decode()
    assert lib.bt_diag_genotype_text(w.ctypes.data, 10, *args) != 0 and "shorter than its tables" in lib.bt_last_error().decode()
    bad = w.copy()
    bad[5 + 5 + 2] = bad[5 + 5 + 3] + 2   # var_off not ascending
    assert lib.bt_diag_genotype_text(bad.ctypes.data, bad.size, *args) != 0 and "offset tables" in lib.bt_last_error().decode()
    bad = w.copy()
    bad[int(w[5 + 5])] = 40   # A of the first variant: its record would end past the next one's start
    assert lib.bt_diag_genotype_text(bad.ctypes.data, bad.size, *args) != 0 and "layout" in lib.bt_last_error().decode()
    bad = w.copy()
    bad[int(w[5 + 5]) + 4 + 4 * 2] = 3   # ploidy 3
    assert lib.bt_diag_genotype_text(bad.ctypes.data, bad.size, *args) != 0 and "layout" in lib.bt_last_error().decode()


# ---- the inputs of the device tests (test_genotype_text_gpu.py) on the host: each meets its stated conditions, and the reference built from Python's '%g'
# ---- alone agrees with the host run of the shared header -------------------------------------------------------------------------------------------------
def _raw_diag(words, text, text_capacity, index, index_capacity):
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    rc = lib.bt_diag_genotype_text(words.ctypes.data, words.size, text, text_capacity, index, index_capacity, C.byref(nt), C.byref(ni), C.byref(nc))
    return rc, nt.value, ni.value, nc.value


@pytest.mark.parametrize("NV,S,multi", SCAN_CASES)
def test_scan_strings_on_the_host(NV, S, multi):
    """the strings that take the device's offsets scan past one workgroup, to its `base + q < num_variants` edges and through NV = 0 and S = 0"""
    words, ref, variants = scan_case(NV, S, multi)
    check_scan_inputs(NV, S, multi, ref, variants)
    text, index, not_covered = lib.diag_genotype_text(words)
    check_against_reference(text, index, not_covered, ref, (NV, S, multi))
    if NV > SCAN_BLOCK:
        at = 5 + ref.Cn + 9 * SCAN_BLOCK
        assert int(index[at]) | (int(index[at + 1]) << 32) == ref.variant_offset(SCAN_BLOCK)
    parsed = lib.parse_genotype_text(text, index)
    assert [p["flags"] for p in parsed] == ref.flags.tolist()
    for v in list(range(min(NV, 3))) + [NV - 1] * (NV > 3):   # (the reference's pieces are expected_pieces' without GQ: a spot check that the two agree)
        if not ref.flags[v]:
            assert (parsed[v]["stats"], parsed[v]["cover"], parsed[v]["samples"]) == expected_pieces(variants[v])


def test_a_malformed_record_past_the_first_scan_block_writes_nothing():
    words, ref, _ = scan_case(2049, 1)
    bad = words.copy()
    bad[ploidy_word(words, 1500)] = 3
    text, index = np.full(ref.text.size, 0xAA, np.uint8), np.full(ref.index.size, 0xAAAAAAAA, np.uint32)
    rc, _, _, _ = _raw_diag(bad, text.ctypes.data, text.size, index.ctypes.data, index.size)
    assert rc != 0 and "layout" in lib.bt_last_error().decode() and (text == 0xAA).all() and (index == 0xAAAAAAAA).all()
    rc, nt, ni, _ = _raw_diag(words, text.ctypes.data, text.size, index.ctypes.data, index.size)   # the string itself is accepted with these buffers
    assert rc == 0 and (nt, ni) == (text.size, index.size)


def test_format_g6_edges_in_records_on_the_host():
    """the values the device test carries into the kernels as k-mer means (doubles) and AF / ACP / GPP / APP (float32)"""
    check_g6_inputs()
    d, f = g6_doubles()["all"], g6_floats()["all"]
    _check_g6(d, "doubles")
    _check_g6(f.astype(np.float64), "floats")
    words, ref = g6_case()
    raw = ref.text.tobytes().decode()
    missing = [x for x in list(d[::97]) + list(f[::53]) if "%g" % float(x) not in raw]   # (make_string placed them: every 97th and 53rd looked up)
    assert not missing and ref.not_covered == 0 and {int(w) for w in ref.index[5 + ref.Cn + 5:5 + ref.Cn + 9 * ref.NV:9]} == set(range(2, 8))
    text, index, not_covered = lib.diag_genotype_text(words)
    check_against_reference(text, index, not_covered, ref, "format_g6 values")


def test_not_covered_values_in_records_on_the_host():
    words, ref, at = not_covered_case()
    assert len(at) == len(g6_not_covered()) == ref.not_covered and np.array_equal(np.flatnonzero(ref.flags), at) and all(b - a == 2 for a, b in zip(at, at[1:]))
    text, index, not_covered = lib.diag_genotype_text(words)
    check_against_reference(text, index, not_covered, ref, "not covered")
    assert [p["flags"] for p in lib.parse_genotype_text(text, index)] == ref.flags.tolist()


def test_store_alignment_on_the_host():
    """StoreSink at every (first byte, one past the last byte) residue, the text at base + 0 .. 3 between guard bytes"""
    words, ref, variants = alignment_case()
    n = ref.text.size
    for shift in range(4):
        buf = np.full(n + 128 + 8, 0xAA, np.uint8)
        start = (-buf.ctypes.data) % 4 + 64 + shift   # base + shift with a 4-aligned base
        assert (buf.ctypes.data + start) % 4 == shift
        check_alignment_inputs(ref, variants, buf.ctypes.data + start)
        index = np.zeros(ref.index.size, np.uint32)
        rc, nt, ni, nc = _raw_diag(words, buf.ctypes.data + start, n, index.ctypes.data, index.size)
        assert rc == 0 and (nt, ni) == (n, index.size)
        check_against_reference(buf[start:start + n], index, nc, ref, f"shift {shift}")
        assert (buf[:start] == 0xAA).all() and (buf[start + n:] == 0xAA).all(), shift
