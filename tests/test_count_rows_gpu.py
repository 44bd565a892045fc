"""Count rows, the merge step of a sharded sample scan, through the C ABI: bt_table_count_row_bytes / bt_table_export_count_rows /
bt_table_merge_count_rows (include/btgpu.h; export_count_rows_kernel and merge_count_rows_kernel).  The reference is a dictionary in numpy: the
tables are filled from numpy records through bt_table_unpack, the rows a merge receives are built in numpy, so what is expected never passes through
the code under test.  Every compare is exact, on rows sorted by key."""
import ctypes as C

import numpy as np
import pytest

import _oracle  # noqa: F401  (sys.path set-up)
from test_table_checkpoint_gpu import K, _keys, _records, _same, _unpack_host

pytestmark = pytest.mark.gpu

SAMPLES = [1, 3, 4, 5, 10, 30]   # count padding 4, 4, 4, 8, 12, 32: the three slot sizes, and a last sample in the last byte of the last word (4)
N_KEYS = 3000


def _spad(S):
    return (S + 3) & ~3


def _designed_counts(rng, n, S):
    """a third of the records all zero, records whose only count is sample 0 / sample S - 1, records holding 255, the rest random; the three special
    keys (the first three of _keys) get counts"""
    c = rng.integers(0, 256, (n, S)).astype(np.uint8)
    kind = rng.permutation(n) % 12
    kind[:3] = (4, 5, 7)
    c[kind < 4] = 0
    for which, col in ((4, 0), (5, S - 1)):
        rows = np.nonzero(kind == which)[0]
        v = c[rows, col] | 1
        c[rows] = 0
        c[rows, col] = v
    rows = np.nonzero(kind == 6)[0]
    c[rows, rng.integers(0, S, len(rows))] = 255
    assert (kind < 4).sum() >= n // 3 - 3 and (c[kind < 4] == 0).all() and (c == 255).any()
    assert ((c[:, 0] != 0) & (c[:, 1:] == 0).all(1)).any() and ((c[:, -1] != 0) & (c[:, :-1] == 0).all(1)).any()
    return c


def _rows(keys, counts, spad):
    """count rows of include/btgpu.h: lo, hi (little endian), the counts padded with zeros to spad; records without a count have no row"""
    keep = (counts != 0).any(1)
    keys, counts = keys[keep], counts[keep]
    r = np.zeros((len(keys), 16 + spad), np.uint8)
    r[:, :16] = np.ascontiguousarray(keys, "<u8").view(np.uint8).reshape(len(keys), 16)
    r[:, 16:16 + counts.shape[1]] = counts
    return r


def _by_key(rows):
    k = np.ascontiguousarray(rows[:, :16]).view("<u8").reshape(len(rows), 2)
    return rows[np.lexsort((k[:, 0], k[:, 1]))]


def _table(ctx, lib, S, expected, keys, counts, meta=None):
    t = lib.Table(ctx, expected, S, K)
    if len(keys):
        _unpack_host(t, _records(keys, np.zeros((len(keys), 4), np.uint8) if meta is None else meta, counts, _spad(S)))
    return t


def _export_into(t, lib, capacity_rows, buffer_rows):
    """bt_table_export_count_rows into a buffer of buffer_rows rows prefilled with 0xA5 -> (return code, *h_num_rows, the buffer's bytes by row)"""
    rb = t.count_row_bytes()
    buf = t.ctx.to_device(np.full(buffer_rows * rb, 0xA5, np.uint8))
    n = C.c_uint64(1 << 60)
    rc = lib.bt_table_export_count_rows(t.h, buf.ptr, capacity_rows, C.byref(n))
    out = buf.download(np.uint8, buffer_rows * rb).reshape(buffer_rows, rb)
    buf.free()
    return rc, n.value, out


def _exported(t):
    buf, n = t.export_count_rows()
    rows = buf.download(np.uint8, n * t.count_row_bytes()).reshape(n, t.count_row_bytes())
    buf.free()
    return rows


def _sized(t, lib):
    n = C.c_uint64(1 << 60)
    lib.check(lib.bt_table_export_count_rows(t.h, None, 0, C.byref(n)))   # d_rows NULL with capacity 0: the sizing call
    return n.value


@pytest.mark.parametrize("S", SAMPLES)
def test_export_count_rows(gpu_ctx, S):
    from bayestyper_amd import lib

    rng = np.random.default_rng(500 + S)
    keys = _keys(rng, N_KEYS)
    counts = _designed_counts(rng, N_KEYS, S)
    meta = rng.integers(0, 256, (N_KEYS, 4)).astype(np.uint8)
    want = _by_key(_rows(keys, counts, _spad(S)))
    n = len(want)
    assert 0 < n == int((counts != 0).any(1).sum()) < N_KEYS
    t = _table(gpu_ctx, lib, S, N_KEYS, keys, counts, meta)
    try:
        assert t.count_row_bytes() == 16 + _spad(S) == want.shape[1]
        assert _sized(t, lib) == n
        # exact capacity: the rows as a set — key bytes, counts, zero padding
        got = _exported(t)
        assert got.shape == want.shape and np.array_equal(_by_key(got), want)
        assert (got[:, 16 + S:] == 0).all()
        # a larger buffer: what lies past n rows is untouched; a second export is the same set
        rc, m, out = _export_into(t, lib, n + 7, n + 7)
        assert rc == 0 and m == n and (out[n:] == 0xA5).all() and np.array_equal(_by_key(out[:n]), want)
        # capacity n - 1: an error, and nothing past the capacity is written
        rc, m, out = _export_into(t, lib, n - 1, n + 3)
        assert rc != 0 and b"too small" in lib.bt_last_error() and (out[n - 1:] == 0xA5).all()
        with pytest.raises(lib.BtError, match="null"):
            lib.check(lib.bt_table_export_count_rows(t.h, None, 5, C.byref(C.c_uint64())))
        # after a rehash into a larger table
        cap = t.status()["capacity"]
        t.reserve(50_000)
        assert t.status()["capacity"] > cap and _sized(t, lib) == n
        assert np.array_equal(_by_key(_exported(t)), want)
        assert _same(t.export(), (keys, counts, meta))   # (and the export left the table as it was)
    finally:
        t.close()


@pytest.mark.parametrize("S", [1, 5])
def test_export_of_tables_without_counts(gpu_ctx, S):
    from bayestyper_amd import lib

    keys = _keys(np.random.default_rng(7), 500)
    for t in (lib.Table(gpu_ctx, 1000, S, K), _table(gpu_ctx, lib, S, 1000, keys, np.zeros((500, S), np.uint8))):
        try:
            assert _sized(t, lib) == 0   # (d_rows NULL is accepted)
            buf, m = t.export_count_rows()
            buf.free()
            assert m == 0
        finally:
            t.close()


def _as_dict(keys, counts, meta):
    return {(int(k[0]), int(k[1])): (c.astype(np.int64), m.copy()) for k, c, m in zip(keys, counts, meta)}


def _merge_ref(table, rows, S):
    """the numpy rule: a row's key is added when absent (zero meta, zero counts); every count byte adds, saturating at 255"""
    keys = np.ascontiguousarray(rows[:, :16]).view("<u8").reshape(len(rows), 2)
    for k, c in zip(keys, rows[:, 16:16 + S]):
        cur = table.setdefault((int(k[0]), int(k[1])), (np.zeros(S, np.int64), np.zeros(4, np.uint8)))
        np.minimum(255, cur[0] + c, out=cur[0])


def _from_dict(d, S):
    keys = np.array(list(d.keys()), np.uint64).reshape(len(d), 2)
    return keys, np.array([v[0] for v in d.values()], np.uint8).reshape(len(d), S), np.array([v[1] for v in d.values()], np.uint8).reshape(len(d), 4)


def _merge(t, rows):
    buf = t.ctx.to_device(rows)
    t.merge_count_rows(buf, len(rows))
    t.ctx.sync()
    buf.free()


def _check(t, ref, S):
    keys, counts, meta = t.export()
    st = t.status()
    assert st["num_keys"] == len(ref) == len(keys) == len(np.unique(keys, axis=0)) and not st["overflowed"]
    assert _same((keys, counts, meta), _from_dict(ref, S))


@pytest.mark.parametrize("S", SAMPLES)
def test_merge_count_rows(gpu_ctx, S):
    from bayestyper_amd import lib

    rng = np.random.default_rng(600 + S)
    all_keys = _keys(rng, N_KEYS + 500)
    src_keys, own_keys = all_keys[:N_KEYS], all_keys[N_KEYS:]
    rows = _rows(src_keys, _designed_counts(rng, N_KEYS, S), _spad(S))
    rows = rows[rng.permutation(len(rows))]
    # the target: half of the source's keys (two of the three special keys among them; the third arrives as a new key) and 500 of its own, with meta bytes and counts of its own
    tgt_keys = np.concatenate([src_keys[::2], own_keys])
    tgt_counts = _designed_counts(rng, len(tgt_keys), S)
    tgt_meta = rng.integers(0, 256, (len(tgt_keys), 4)).astype(np.uint8)
    ref = _as_dict(tgt_keys, tgt_counts, tgt_meta)
    t = _table(gpu_ctx, lib, S, 8000, tgt_keys, tgt_counts, tgt_meta)
    try:
        _check(t, ref, S)
        _merge(t, rows)
        _merge_ref(ref, rows, S)
        assert len(ref) > len(tgt_keys) and any((v[0] == 255).any() for v in ref.values())
        _check(t, ref, S)
        _merge(t, rows)   # the same rows again: a + 2b, saturating
        _merge_ref(ref, rows, S)
        _check(t, ref, S)
        lib.check(lib.bt_table_merge_count_rows(t.h, None, 0))   # no rows, NULL: a no-op
        gpu_ctx.sync()
        _check(t, ref, S)
        with pytest.raises(lib.BtError, match="null"):
            lib.check(lib.bt_table_merge_count_rows(t.h, None, 3))
    finally:
        t.close()


@pytest.mark.parametrize("S", SAMPLES)
def test_merge_under_contention(gpu_ctx, S):
    """the add is a compare-and-swap loop on the count word: rows of one key that meet in one launch lose nothing"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(700 + S)
    keys = _keys(rng, N_KEYS + 2)
    rows = _rows(keys[:N_KEYS], _designed_counts(rng, N_KEYS, S), _spad(S))
    ref = {}
    t = lib.Table(gpu_ctx, 8000, S, K)
    try:
        # every row twice in one batch, shuffled
        twice = np.concatenate([rows, rows])[rng.permutation(2 * len(rows))]
        _merge(t, twice)
        _merge_ref(ref, twice, S)
        _check(t, ref, S)
        # 64 consecutive copies of one row: the lanes of one wavefront add to the same bytes
        one = _rows(keys[N_KEYS:N_KEYS + 1], np.array([[1, 3, 4, 200][s % 4] for s in range(S)], np.uint8)[None], _spad(S))
        same = np.repeat(one, 64, axis=0)
        _merge(t, same)
        _merge_ref(ref, same, S)
        want = np.minimum(255, 64 * one[0, 16:16 + S].astype(np.int64))
        assert np.array_equal(ref[tuple(int(x) for x in keys[N_KEYS])][0], want) and (want == 64).any()
        _check(t, ref, S)
        # 64 consecutive rows of one key, each non-zero in another sample column of the same count word
        cols = min(S, 4)
        c = np.zeros((64, S), np.uint8)
        c[np.arange(64), np.arange(64) % cols] = 1 + np.arange(64) % 7
        cross = _rows(np.repeat(keys[N_KEYS + 1:], 64, axis=0), c, _spad(S))
        assert len(cross) == 64
        _merge(t, cross)
        _merge_ref(ref, cross, S)
        assert np.array_equal(ref[tuple(int(x) for x in keys[N_KEYS + 1])][0][:cols], c.astype(np.int64).sum(0)[:cols])
        _check(t, ref, S)
    finally:
        t.close()


def test_merge_overflow_is_reported(gpu_ctx):
    """5 000 new keys into a table created for 16 (as the insert overflow of test_kmer_gpu.py::test_error_paths_report_instead_of_computing):
    the overflow is latched and reported by bt_table_status, and bt_table_reserve refuses the table"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(3)
    keys = _keys(rng, 5000)
    rows = _rows(keys, rng.integers(1, 256, (5000, 3)).astype(np.uint8), 4)
    small = lib.Table(gpu_ctx, 16, 3, K)
    try:
        assert not small.status()["overflowed"]
        _merge(small, rows)
        st = small.status()
        assert st["overflowed"] and st["num_keys"] <= st["capacity"] < len(keys)
        got = _by_key(_exported(small))
        assert len(got) == st["num_keys"] and len(np.unique(got[:, :16], axis=0)) == len(got)   # what it holds, it holds once and with a count
        with pytest.raises(lib.BtError):
            small.reserve(10_000)
    finally:
        small.close()
