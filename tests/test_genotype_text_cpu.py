"""The genotype text of the device route without a GPU: bt_diag_format_g6 and bt_diag_genotype_text run the __host__ __device__ code of the text kernels
(bayestyper_amd/csrc/bt_genotype_text.hpp) on the host.  The number formatter against Python's '%g' (correctly rounded, as glibc's printf), the three pieces of
every variant against the host layer's stream formatters, byte for byte.  All of it fails without the text entries."""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle
from _genotype_text import assert_cluster_text_equals_host, expected_pieces, hand_written, make_string
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
    from fractions import Fraction

    ties = []
    for p in range(6):
        for D in list(range(100000, 100400)) + list(range(524280, 524300)) + list(range(999600, 1000000)) + list(range(123456, 999999, 7919)):
            v = (D + 0.5) / 10 ** p
            if Fraction(v) == Fraction(2 * D + 1, 2 * 10 ** p):
                ties.append(v)
    assert len(ties) > 1000   # (p = 0 always; p >= 1 when (2 D + 1) / 2 is a multiple of 5^p)
    assert sum(1 for v in ties if v != math.floor(v) + 0.5) > 10
    _check_g6(ties, "ties")
    # near both notation switches: 10^-5 | 10^-4 (exponent / fixed) and 10^5 | 10^6 (fixed / exponent)
    near = [D * 10.0 ** p + 0.5 * 10.0 ** p for p in (-10, -9, -1, 0) for D in (99999, 100000, 999999, 999998, 123456)]
    got = _check_g6(near, "switches")
    assert got[near.index(999999 + 0.5)] == "1e+06" and got[5].endswith("e-05") and got[6].startswith("0.0001") and got[near.index(99999.5)] == "99999.5"


def test_range_edges():
    edges = [9.9999949e-5, 9.9999951e-5, 1e-4, 999999.4, 999999.5, 1e-27, -1.0, 0.0, -0.0, 1.0, 0.5, -0.25, 100000.0, 123456.0]
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
