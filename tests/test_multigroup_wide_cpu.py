"""CPU tests of the staged k-mer-set order behind the workgroup route of bt_paths_count_multigroup (mg_order_wide_kernel): the same
__host__ __device__ code run by a team of one host thread (bt_diag_kmer_set_order_staged) against the real container of the reference
(oracle/_ref/libbtref.so) and against the insert-by-insert replay (bt_diag_kmer_set_order).  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _oracle  # noqa: E402
import mg_wide_groups as MG  # noqa: E402

K = MG.K


def _staged(lib, packed, buckets):
    n = len(packed)
    rank = np.zeros(max(n, 1), np.uint32)
    final = C.c_uint64(0)
    lib.check(lib.bt_diag_kmer_set_order_staged(packed.ctypes.data if n else rank.ctypes.data, n, buckets, K, rank.ctypes.data, C.byref(final)))
    return rank[:n], final.value


def test_staged_order_vs_reference_container(oracle, ref):
    """One sequence of groups through one container, the bucket count inherited from group to group: sizes that straddle the first rehash
    points (13/14, 29/30, 59/60), groups with several stages (700, 5 000, 30 000, 70 000), small groups that inherit many buckets (a single
    stage), empty groups.  The staged order and the stage plan's bucket count equal the real container's, group by group.  The sequence
    hands the 70 000 group 42 043 buckets, which leaves it two stages; it is therefore also run alone in a fresh set, where it passes
    through all 13 bucket counts from 13 to 85 229."""
    from bayestyper_amd import lib

    seq = MG.group_sequence(oracle, ref)
    buckets = 1
    for g, packed in enumerate(seq["packed"]):
        rank, final = _staged(lib, packed, buckets)
        assert np.array_equal(MG.order_of(rank), seq["order"][g]), f"group {g} ({len(packed)} k-mers, {buckets} buckets inherited)"
        assert final == int(seq["buckets"][g]), (g, final, int(seq["buckets"][g]))
        buckets = final
    assert buckets == 85229
    rank, final = _staged(lib, seq["packed"][MG.BIG], 1)
    assert np.array_equal(MG.order_of(rank), seq["fresh_order"]) and final == seq["fresh_buckets"] == 85229


def test_stage_plan_and_staged_ranks_vs_replay(oracle):
    """n in 0..300 and at 1109/1110, 2357/2358 (around two later rehash points), containers that start with 1, 13, 29, 127 or 85 229
    buckets: the stage plan ends at the replay's bucket count, and the staged ranks are the replay's ranks."""
    from bayestyper_amd import lib

    rng = np.random.default_rng(77)
    pool = np.unique(_oracle.random_kmers(rng, 2358, K).reshape(-1, K), axis=0)
    pool = pool[rng.permutation(len(pool))]
    assert len(pool) == 2358
    packed_all = np.ascontiguousarray(oracle.pack(np.ascontiguousarray(pool).reshape(-1), K), np.uint64).reshape(-1, 2)
    for n in list(range(301)) + [1109, 1110, 2357, 2358]:
        packed = np.ascontiguousarray(packed_all[:n])
        for buckets in (1, 13, 29, 127, 85229):
            rank, final = _staged(lib, packed, buckets)
            want = np.zeros(max(n, 1), np.uint32)
            want_final = C.c_uint64(0)
            lib.check(lib.bt_diag_kmer_set_order(packed.ctypes.data if n else want.ctypes.data, n, buckets, K, want.ctypes.data, C.byref(want_final)))
            assert final == want_final.value, (n, buckets, final, want_final.value)
            assert np.array_equal(rank, want[:n]), (n, buckets)


def test_staged_order_rejects_bucket_counts_beyond_32_bits(oracle):
    """the stage code numbers buckets in 32 bits: a container of 2^32 - 2 buckets or more is an error, as on the device route, not a wrong order"""
    from bayestyper_amd import lib

    packed = np.ascontiguousarray(oracle.pack(_oracle.random_kmers(np.random.default_rng(1), 3, K), K), np.uint64)
    rank = np.zeros(3, np.uint32)
    for buckets in (0xFFFFFFFE, 1 << 32, 1 << 40):
        assert lib.bt_diag_kmer_set_order_staged(packed.ctypes.data, 3, buckets, K, rank.ctypes.data, None) != 0
    lib.check(lib.bt_diag_kmer_set_order_staged(packed.ctypes.data, 3, 0xFFFFFFFD, K, rank.ctypes.data, None))
    assert sorted(rank) == [0, 1, 2]
