"""CPU tests of the k-dependent host code at k-mer sizes other than 55: the restatements of std::hash<std::bitset<2k>> (bthost::bitsetHash,
the library's std_hash_bitset) against the standard library's own hash at every k in 1..64; both replays of the multigroup pass's container
against the real std::unordered_set<std::bitset<2k>> the oracle instantiates at run-time k (_oracle.KMER_SET_SIZES); the parameter k-mer
order against the reference built at k = 31 and 64 (oracle/_ref/libbtref_k31.so, libbtref_k64.so); the host graph constructor at k = 15, 32
and 64.  Every comparison is exact.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _oracle  # noqa: E402
import mg_wide_groups as MG  # noqa: E402
import test_host_graph_cpu as HG  # noqa: E402

KS = list(_oracle.KMER_SET_SIZES)
# 13/14, 29/30 and 59/60 straddle the first rehash points of the prime chain; 700 and 5 000 grow through several bucket counts inside a group;
# 3 and 9 inherit many buckets
GROUP_SIZES = [0, 1, 12, 13, 14, 29, 30, 59, 60, 700, 3, 5000, 9]


def group_sizes(k):
    """the group sizes of the order tests: k = 3 has 64 distinct k-mers only, so its list ends at 60"""
    return GROUP_SIZES[:GROUP_SIZES.index(60) + 1] if k == 3 else GROUP_SIZES


def distinct_kmers(rng, n, k):
    """n distinct random ASCII k-mers [n, k], in random order"""
    nt = np.frombuffer(b"ACGT", np.uint8)
    if 4 ** k <= 4096:
        codes = rng.permutation(4 ** k)[:n]
        assert len(codes) == n
        return nt[(codes[:, None] >> (2 * np.arange(k))) & 3].reshape(n, k)
    km = np.zeros((0, k), np.uint8)
    while len(km) < n:
        km = np.concatenate([km, nt[rng.integers(0, 4, (n + 8, k))]])
        km = km[np.sort(np.unique(km, axis=0, return_index=True)[1])]
    return np.ascontiguousarray(km[:n])


def kmer_groups(oracle, k, sizes, seed=None):
    """(ASCII groups, packed groups) of distinct k-mers of the given sizes"""
    rng = np.random.default_rng(20270 + k if seed is None else seed)
    groups = [distinct_kmers(rng, n, k) for n in sizes]
    packed = [np.ascontiguousarray(oracle.pack(np.ascontiguousarray(g).reshape(-1), k), np.uint64).reshape(-1, 2) if len(g) else np.zeros((0, 2), np.uint64)
              for g in groups]
    return groups, packed


def _hash_inputs(rng, k):
    """1000 random k-mers, all-zero, all-ones under the 2k-bit mask and the single top bit, as (lo, hi)"""
    mask = (1 << (2 * k)) - 1
    vals = [int(a) | (int(b) << 64) for a, b in rng.integers(0, 2 ** 64, (1000, 2), dtype=np.uint64)]
    vals = [v & mask for v in vals] + [0, mask, 1 << (2 * k - 1)]
    return [(v & (2 ** 64 - 1), v >> 64) for v in vals]


@pytest.mark.parametrize("k", range(1, 65))
def test_bitset_hash_restatements_vs_standard_library(oracle, k):
    """bthost::bitsetHash (the parameter k-mer order's root bucket) and the library's std_hash_bitset (the multigroup replay's bucket) equal
    std::hash<std::bitset<2k>> of the standard library the oracle is built with: the hashed length (2k + 7) / 8 bytes has no whole word for
    k <= 31, exactly one word and no tail at k = 29..32, a tail in the second word at k = 33..60 and two whole words from k = 61"""
    from bayestyper_amd import lib
    from bayestyper_amd.host import dll

    dll.bth_bitset_hash.restype = C.c_uint64
    dll.bth_bitset_hash.argtypes = [C.c_uint64, C.c_uint64, C.c_uint]
    for lo, hi in _hash_inputs(np.random.default_rng(1000 + k), k):
        want = oracle.std_hash_bitset(lo, hi, k)
        assert dll.bth_bitset_hash(lo, hi, k) == want, (k, hex(lo), hex(hi))
        assert lib.bt_diag_std_hash_bitset(lo, hi, k) == want, (k, hex(lo), hex(hi))


def _replays(lib):
    return (("bt_diag_kmer_set_order", lib.bt_diag_kmer_set_order), ("bt_diag_kmer_set_order_staged", lib.bt_diag_kmer_set_order_staged))


@pytest.mark.parametrize("k", KS)
def test_kmer_set_orders_vs_real_container(oracle, k):
    """One std::unordered_set<std::bitset<2k>> per k, carried through GROUP_SIZES with its bucket count inherited from group to group:
    the insert-by-insert replay and the staged order give the real container's iteration order and bucket count, group by group.  Where
    the reference is built at this k (31, 55, 64), its own container filled through Nucleotide::ntToBit gives the same orders."""
    from bayestyper_amd import lib

    groups, packed = kmer_groups(oracle, k, group_sizes(k))
    want_order, want_buckets = oracle.kmer_set_orders(k, groups)
    for name, fn in _replays(lib):
        buckets = 1
        for g, pk in enumerate(packed):
            n = len(pk)
            rank = np.zeros(max(n, 1), np.uint32)
            final = C.c_uint64(0)
            lib.check(fn(pk.ctypes.data if n else rank.ctypes.data, n, buckets, k, rank.ctypes.data, C.byref(final)))
            assert np.array_equal(MG.order_of(rank[:n]), want_order[g]), f"{name}, k = {k}, group {g} ({n} k-mers, {buckets} buckets inherited)"
            assert final.value == int(want_buckets[g]), (name, k, g, final.value, int(want_buckets[g]))
            buckets = final.value
        assert buckets == (127 if k == 3 else 5087)
    ref = _oracle.load_ref(k)
    if ref is not None:
        ref_order, ref_buckets = MG.ref_orders(ref, groups)
        assert np.array_equal(ref_buckets, want_buckets)
        for g in range(len(groups)):
            assert np.array_equal(ref_order[g], want_order[g]), (k, g)


def test_oracle_container_vs_reference_at_55(oracle, ref):
    """orc_kmer_set_orders at k = 55 equals ref_group_kmer_set_orders of the reference as it is built, on the group sequence of the multigroup
    tests (rehash points, 70 000 k-mers in one group, small groups that inherit many buckets)"""
    seq = MG.group_sequence(oracle, ref)
    groups = [oracle.unpack(p, MG.K).reshape(-1, MG.K) for p in seq["packed"]]
    order, buckets = oracle.kmer_set_orders(MG.K, groups)
    assert np.array_equal(buckets, seq["buckets"])
    for g in range(len(groups)):
        assert np.array_equal(order[g], seq["order"][g]), g
    order, buckets = oracle.kmer_set_orders(MG.K, [groups[MG.BIG]])
    assert np.array_equal(order[0], seq["fresh_order"]) and int(buckets[0]) == seq["fresh_buckets"]
    # a set that starts with inherited buckets: the tail of the sequence alone, from the bucket count the group before it left
    g0 = MG.SIZES.index(30000) + 1
    order, buckets = oracle.kmer_set_orders(MG.K, groups[g0:], initial_buckets=int(seq["buckets"][g0 - 1]))
    assert np.array_equal(buckets, seq["buckets"][g0:])
    for g in range(g0, len(groups)):
        assert np.array_equal(order[g - g0], seq["order"][g]), g


def test_oracle_refuses_a_size_without_a_container(oracle):
    """a k outside KMER_SET_SIZES is an error in orc_kmer_set_orders and in OrcGraphs.count_multigroup: no other container has the order"""
    from bayestyper_amd import synth_graphs

    for k in (16, 54, 56):
        assert k not in KS
        with pytest.raises(ValueError, match="unordered_set"):
            oracle.kmer_set_orders(k, [distinct_kmers(np.random.default_rng(k), 5, k)])
        f = synth_graphs.flatten([synth_graphs.random_cluster(np.random.default_rng(k), k, 2, 2)])
        og, ob, ot = _oracle.OrcGraphs(oracle, f, k), _oracle.OrcBloom(oracle, 1000, 1e-3, k), _oracle.OrcTable(oracle, 1, k)
        with pytest.raises(ValueError, match="count_multigroup"):
            og.count_multigroup(np.zeros(1, np.uint32), ob, ot)
        assert oracle.l.orc_paths_count_multigroup(og.h, np.zeros(1, np.uint32).ctypes.data, ob.h, ot.h) == 2 ** 64 - 1
        for x in (og, ob, ot):
            x.close()
    with pytest.raises(ValueError, match="does not take"):
        oracle.kmer_set_orders(31, [distinct_kmers(np.random.default_rng(1), 5, 31)], initial_buckets=100)


@pytest.mark.parametrize("root_size,n", [(4 ** 12, 20000), (64, 3000), (1, 300)])
@pytest.mark.parametrize("k", [31, 64])
def test_parameter_kmer_order_vs_reference(oracle, k, root_size, n):
    """bthost::hybridHashShuffledOrder against the reference's own HybridHash built at k = 31 and k = 64 (the body of
    test_host_cli_cpu.py::test_parameter_kmer_order_vs_reference): the real 4^12 roots, and tiny root tables where every leaf holds many
    k-mers.  The reference compiles at 64, so no smaller size stands in for it."""
    from bayestyper_amd.host import dll

    ref = _oracle.load_ref(k)
    if ref is None:
        pytest.skip(f"{os.path.relpath(_oracle.ref_so(k), ROOT)} not built (needs the reference tree)")
    dll.bth_bitset_hash.restype = C.c_uint64
    dll.bth_bitset_hash.argtypes = [C.c_uint64, C.c_uint64, C.c_uint]
    dll.bth_hybrid_hash_order.argtypes = [C.c_void_p, C.c_uint64, C.c_uint, C.c_uint, C.c_uint64, C.c_void_p]
    rng = np.random.default_rng(n + k)
    km = distinct_kmers(rng, n, k)
    flat = np.ascontiguousarray(km).reshape(-1)
    ref.l.ref_hybrid_hash_order.restype = C.c_uint64
    ref.l.ref_hybrid_hash_order.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint, C.c_int, C.c_void_p]
    packed = np.ascontiguousarray(oracle.pack(flat, k), np.uint64)
    for seed, shuffle in ((42, 1), (7, 1), (0, 0)):
        want = np.zeros(n, np.uint32)
        assert ref.l.ref_hybrid_hash_order(flat.ctypes.data, n, root_size, seed, shuffle, want.ctypes.data) == n
        if shuffle:
            got = np.zeros(n, np.uint32)
            dll.bth_hybrid_hash_order(packed.ctypes.data, n, k, seed, root_size, got.ctypes.data)
            assert np.array_equal(got, want)
        else:   # unshuffled iteration: root order, then BitsetLess = the 2k-bit value ascending
            roots = np.array([dll.bth_bitset_hash(int(a), int(b), k) % root_size for a, b in packed.reshape(-1, 2)], np.uint64)
            p = packed.reshape(-1, 2)
            assert np.array_equal(want, np.lexsort((p[:, 0], p[:, 1], roots)).astype(np.uint32))


@pytest.mark.parametrize("k", [15, 32, 64])
def test_host_graph_constructor(k):
    """bthost::VariantClusterGraph at k = 15, 32 and 64 against synth_graphs.build_graph and against the oracle's restatement of the
    reference constructor, on the inputs of test_host_graph_cpu.py: the flank lengths, the nested cuts and the N-run splits all move with k"""
    HG.check_cpp_graph_equals_python_restatement(k)
    HG.check_cpp_graph_equals_oracle_restatement(k)
