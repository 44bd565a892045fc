"""Shared input of test_multigroup_wide_cpu.py / test_multigroup_wide_gpu.py: one sequence of k-mer groups that go through ONE
std::unordered_set (clear()ed between groups, so the bucket count is inherited), and the iteration orders and bucket counts the real
container gives them (ref_group_kmer_set_orders of oracle/_ref/libbtref.so: the reference's k-mer encoding filling a real
unordered_set<bitset<110>>).  Computed once per test session and never modified."""
import ctypes as C
import functools

import numpy as np

import _oracle

K = 55
# 13/14, 29/30 and 59/60 straddle the first rehash points of the prime chain; the small groups after 5 000, 30 000 and 70 000 have a single
# stage with inherited buckets; 70 000 crosses 2^16
SIZES = [0, 1, 2, 5, 11, 12, 13, 14, 28, 29, 30, 59, 60, 700, 3, 5000, 1, 17, 30000, 12, 100, 70000, 9]
BIG = SIZES.index(70000)


def ref_orders(ref, groups):
    """(order, buckets) of the real container over `groups` (ASCII arrays [n, K]): order[g][j] = the k-mer of group g visited j-th"""
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
    flat = np.ascontiguousarray(np.concatenate(groups)).reshape(-1)
    want_order = np.zeros(max(int(off[-1]), 1), np.uint32)
    want_buckets = np.zeros(len(groups), np.uint64)
    ref.l.ref_group_kmer_set_orders.restype = None
    ref.l.ref_group_kmer_set_orders.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    ref.l.ref_group_kmer_set_orders(flat.ctypes.data, off.ctypes.data, len(groups), want_order.ctypes.data, want_buckets.ctypes.data)
    return [want_order[int(off[g]):int(off[g + 1])] for g in range(len(groups))], want_buckets


def order_of(rank):
    """ranks (position of k-mer i in the iteration order) -> order (the k-mer visited j-th)"""
    order = np.zeros(len(rank), np.uint32)
    order[rank] = np.arange(len(rank), dtype=np.uint32)
    return order


@functools.lru_cache(maxsize=None)
def _cached(oracle, ref):
    rng = np.random.default_rng(20261)
    groups = []
    for n in SIZES:
        km = np.unique(_oracle.random_kmers(rng, n, K).reshape(-1, K), axis=0) if n else np.zeros((0, K), np.uint8)
        groups.append(km[rng.permutation(len(km))])
    assert [len(g) for g in groups] == SIZES   # (random 55-mers do not collide)
    packed = [np.ascontiguousarray(oracle.pack(np.ascontiguousarray(g).reshape(-1), K), np.uint64).reshape(-1, 2) if len(g) else np.zeros((0, 2), np.uint64)
              for g in groups]
    order, buckets = ref_orders(ref, groups)
    # the largest group alone in a freshly constructed set: every stage of the prime chain from 13 buckets up (the sequence above hands it 42 043 buckets,
    # which leaves it two stages)
    fresh_order, fresh_buckets = ref_orders(ref, [groups[BIG]])
    for a in packed + order + [buckets, fresh_order[0], fresh_buckets]:
        a.setflags(write=False)
    return {"packed": packed, "order": order, "buckets": buckets, "fresh_order": fresh_order[0], "fresh_buckets": int(fresh_buckets[0])}


def group_sequence(oracle, ref):
    return _cached(oracle, ref)
