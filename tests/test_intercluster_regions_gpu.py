"""bt_table_count_intercluster_regions (intercluster_regions_kernel: every region of a sequence in one launch, tiled by RegionTile) against the oracle's
region-by-region walk (OrcTable.count_intercluster once per region; the update is commutative), through the C ABI.  In the same file the two bound
entry points no test called: bt_table_read_slots and bt_bloom_clear."""
import ctypes as C

import numpy as np
import pytest

import _oracle
from _oracle import OrcBloom, OrcTable
from test_table_checkpoint_gpu import _keys, _records, _unpack_host

pytestmark = pytest.mark.gpu

TILE = 1024   # SEQ_TILE of bt_table.hip: k-mer start positions per tile
L = 40_000
PLOIDIES = [(2, 2), (2, 1), (1, 1), (0, 1)]


def _genome():
    rng = np.random.default_rng(31)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy()
    g[5000:5010] = ord("N")
    g[7020:7030] = ord("N")                               # straddles position 1024 of the region that starts at 6000
    g[9000:9300] += 32                                    # lower case
    g[20_000:28_000] = g[10_000:18_000]                   # a repeat
    g[30_000:30_400] = ord("A")                           # poly-A: one k-mer passes 127 and 255 occurrences
    return g


def _regions(k):
    """(start, length, decoy, female ploidy, male ploidy) of one call"""
    rng = np.random.default_rng(1000 + k)
    where = [(0, 1025),                                                          # starts on the first nucleotide
             (1100, 0), (1200, 1), (1300, k - 1), (1400, k), (1500, k + 1),
             (2000, 1023),
             (3100, 1024), (4124, 1024 + k - 2),                                 # adjacent: no k-mer across the seam at 4124; the second holds the first N run
             (6000, 2 * TILE + k - 1),                                           # the second N run lies across its first tile seam
             (8500, 1024 + k - 1),                                               # holds the lower-case stretch
             (10_000, 1024 + k), (10_500, 1025),                                 # overlapping: counted twice
             (20_000, 1500),                                                     # in the copy of the repeat
             (29_000, 3 * TILE + 7), (29_900, 1024),                             # both hold the poly-A stretch
             (L - 1029, 1029)]                                                   # ends on the last nucleotide
    short = [(int(s), int(n)) for s, n in zip(rng.integers(32_100, 38_800, 3000), rng.integers(56, 81, 3000))]
    flags = [(int(rng.integers(0, 4) == 0),) + PLOIDIES[int(rng.integers(0, 4))] for _ in range(len(where) + len(short))]
    flags[7], flags[8] = (0, 2, 1), (0, 2, 1)
    flags[14], flags[15] = (0, 2, 2), (0, 2, 1)          # the poly-A k-mer is counted on a chromosome: its multiplicities saturate
    regs = [w + f for w, f in zip(where + short, flags)]
    lens = {n for _, n, *_ in regs}
    assert {0, 1, k - 1, k, k + 1, 1023, 1024, 1025, 1024 + k - 2, 1024 + k - 1, 1024 + k, 2048 + k - 1, 3 * 1024 + 7} <= lens
    assert all(s + n <= L for s, n, *_ in regs) and any(s + n == L for s, n, *_ in regs) and any(s == 0 for s, *_ in regs)
    assert {f[1:] for f in flags} == set(PLOIDIES) and {f[0] for f in flags} == {0, 1}
    return regs


_REFERENCE = {}


def _reference(oracle, k):
    """the path k-mers (about half of the genome's) and the oracle's table after the region-by-region walk: computed once per k"""
    if k not in _REFERENCE:
        g = _genome()
        km, valid = oracle.kmers_from_sequence(g.tobytes(), k)
        pick = (valid == 1) & (np.random.default_rng(77).random(L) < 0.5)
        pick[30_000 + k - 1:30_400] = True                # the poly-A k-mer is a path k-mer
        path = np.unique(km[pick], axis=0)
        ob = OrcBloom(oracle, len(path), 1e-2, k, threaded=True)
        ob.insert(oracle.unpack(path, k))
        ot = OrcTable(oracle, 1, k)
        for start, n, decoy, f, m in _regions(k):
            ot.count_intercluster(ob, g[start:start + n].tobytes(), decoy, f, m)
        wk, _, wm = ot.export()
        order = np.lexsort((wk[:, 0], wk[:, 1]))
        ob.close(), ot.close()
        _REFERENCE[k] = (path, wk[order], wm[order])
    return _REFERENCE[k]


def _keys_meta(t):
    k, c, m = t.export()
    assert not c.any()
    order = np.lexsort((k[:, 0], k[:, 1]))
    return k[order], m[order]


@pytest.mark.parametrize("S", [1, 10])
@pytest.mark.parametrize("k", [31, 32, 33, 55, 64])
def test_regions_in_one_launch(gpu_ctx, oracle, k, S):
    from bayestyper_amd import lib

    g = _genome()
    regs = _regions(k)
    path, wk, wm = _reference(oracle, k)
    num_tiles = sum((n + TILE - 1) // TILE for _, n, *_ in regs)
    assert num_tiles > 8 * gpu_ctx.info()["num_cu"]       # more tiles than the launch has workgroups: the stride loop runs
    assert (wm[:, 0] & 0x10).any() and (wm[:, 0] & 0x08).any() and (wm[:, 1:] == 255).all(1).any() and (wm[:, 2] >= 4).any() and len(wk) > 5000
    assert not {tuple(x) for x in wk.tolist()} <= {tuple(x) for x in path.tolist()}   # Bloom false positives among the keys
    cols = [np.array(c) for c in zip(*regs)]
    gb = lib.Bloom.create(gpu_ctx, len(path), 1e-2, k, threaded=True)
    gb.insert(path)
    other = lib.Bloom.create(gpu_ctx, 100, 1e-2, k + 1 if k < 64 else 63, threaded=True)
    t, one = lib.Table(gpu_ctx, 60_000, S, k), lib.Table(gpu_ctx, 60_000, S, k)
    d_seq = gpu_ctx.to_device(g)
    try:
        t.count_intercluster_regions(gb, g.tobytes(), *cols)
        gk, gm = _keys_meta(t)
        assert not t.status()["overflowed"]
        assert np.array_equal(gk, wk)
        assert np.array_equal(gm, wm)
        # the device's own one-region calls
        for start, n, decoy, f, m in regs:
            lib.check(lib.bt_table_count_intercluster(one.h, gb.h, d_seq.ptr + start, n, decoy, f, m))
        gpu_ctx.sync()
        ok, om = _keys_meta(one)
        assert np.array_equal(ok, gk) and np.array_equal(om, gm)
        # no regions: nothing happens, with or without arrays
        t.count_intercluster_regions(gb, g.tobytes(), *[c[:0] for c in cols])
        lib.check(lib.bt_table_count_intercluster_regions(t.h, gb.h, d_seq.ptr, 0, None, None, None, None, None))
        # errors leave the table alone
        a = [np.ascontiguousarray(cols[0], np.uint64), np.ascontiguousarray(cols[1], np.uint64)] + [np.ascontiguousarray(c, np.uint8) for c in cols[2:]]
        for missing in range(5):
            ptrs = [None if i == missing else x.ctypes.data_as(C.c_void_p) for i, x in enumerate(a)]
            with pytest.raises(lib.BtError, match="null argument"):
                lib.check(lib.bt_table_count_intercluster_regions(t.h, gb.h, d_seq.ptr, len(regs), *ptrs))
        with pytest.raises(lib.BtError, match="k mismatch"):
            t.count_intercluster_regions(other, g.tobytes(), *cols)
        k2, m2 = _keys_meta(t)
        assert np.array_equal(k2, gk) and np.array_equal(m2, gm)
    finally:
        d_seq.free()
        for x in (t, one, gb, other):
            x.close()


def test_read_slots(gpu_ctx):
    """find, then bt_table_read_slots, gives the records the table was filled with; a slot outside the table reads as zeros"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(41)
    S = 5
    keys = _keys(rng, 200)
    counts = rng.integers(0, 256, (200, S)).astype(np.uint8)
    meta = rng.integers(0, 256, (200, 4)).astype(np.uint8)
    t = lib.Table(gpu_ctx, 1000, S, 55)
    try:
        _unpack_host(t, _records(keys, meta, counts, 8))
        slots = t.find(keys)
        cap = t.status()["capacity"]
        assert (slots >= 0).all() and (slots < cap).all() and len(np.unique(slots)) == 200
        c, m = t.read_slots(slots)
        assert np.array_equal(c, counts) and np.array_equal(m, meta)
        ek, ec, em = t.export()
        pos = {tuple(x): i for i, x in enumerate(ek.tolist())}
        order = [pos[tuple(x)] for x in keys.tolist()]
        assert np.array_equal(ec[order], c) and np.array_equal(em[order], m)
        # slot -1 (find's "absent") and slot `capacity`, between good ones: zeros, written over whatever the arrays held
        mixed = np.array([slots[0], -1, slots[1], cap, slots[2]], np.int64)
        c = np.full((5, S), 0xA5, np.uint8)
        m = np.full((5, 4), 0xA5, np.uint8)
        lib.check(lib.bt_table_read_slots(t.h, mixed.ctypes.data_as(C.c_void_p), 5, c.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(c[[0, 2, 4]], counts[:3]) and np.array_equal(m[[0, 2, 4]], meta[:3])
        assert not c[[1, 3]].any() and not m[[1, 3]].any()
    finally:
        t.close()


@pytest.mark.parametrize("threaded", [False, True])
def test_bloom_clear(gpu_ctx, oracle, threaded):
    """after bt_bloom_clear every bit is zero and nothing is contained; inserting again gives the oracle's bits"""
    from bayestyper_amd import lib

    k = 55
    rng = np.random.default_rng(43)
    members = _oracle.random_kmers(rng, 3000, k)
    packed = oracle.pack(members, k)
    ob = OrcBloom(oracle, 3000, 1e-2, k, threaded=threaded)
    ob.insert(members)
    gb = lib.Bloom.create(gpu_ctx, 3000, 1e-2, k, threaded=threaded)
    try:
        subs = range(gb.info()["num_sub"]) if not threaded else sorted({0, 65535} | {ob.route(members[i * k:(i + 1) * k].tobytes()) for i in range(20)})
        gb.insert(packed)
        assert all(np.array_equal(gb.bits(s), ob.bits(s)) for s in subs) and any(gb.bits(s).any() for s in subs) and gb.contains(packed).all()
        lib.check(lib.bt_bloom_clear(gb.h))
        gpu_ctx.sync()
        assert not any(gb.bits(s).any() for s in subs) and not gb.contains(packed).any()
        gb.insert(packed)
        assert all(np.array_equal(gb.bits(s), ob.bits(s)) for s in subs) and gb.contains(packed).all()
    finally:
        gb.close()
        ob.close()
