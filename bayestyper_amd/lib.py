"""ctypes binding of libbtgpu.so (include/btgpu.h).  No fallback: a missing library is an ImportError."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BTGPU_LIB", os.path.join(_HERE, "libbtgpu.so"))   # BTGPU_LIB: alternative build of the same library (tuning experiments)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
        "or bayestyper_amd/csrc/build.sh). There is no CPU fallback."
    )

_lib = C.CDLL(LIB_PATH)

u8p, u32p, u64p, i64p, f64p, f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_int64, C.c_double, C.c_float))
vp = C.c_void_p


def _sig(name, argtypes, restype=C.c_int):
    f = getattr(_lib, name)
    f.argtypes = argtypes
    f.restype = restype
    return f


bt_last_error = _sig("bt_last_error", [], C.c_char_p)
bt_version = _sig("bt_version", [])
bt_device_count = _sig("bt_device_count", [C.POINTER(C.c_int)])
bt_ctx_create = _sig("bt_ctx_create", [C.c_int, C.POINTER(vp)])
bt_ctx_destroy = _sig("bt_ctx_destroy", [vp])
bt_ctx_set_stream = _sig("bt_ctx_set_stream", [vp, vp])
bt_ctx_use_default_stream = _sig("bt_ctx_use_default_stream", [vp])
bt_sync = _sig("bt_sync", [vp])
bt_ctx_info = _sig("bt_ctx_info", [vp, C.POINTER(C.c_int), u64p, u64p, C.c_char_p, C.c_size_t])
bt_malloc = _sig("bt_malloc", [vp, C.c_size_t, C.POINTER(vp)])
bt_free = _sig("bt_free", [vp, vp])
bt_memset = _sig("bt_memset", [vp, vp, C.c_int, C.c_size_t])
bt_memcpy_h2d = _sig("bt_memcpy_h2d", [vp, vp, vp, C.c_size_t])
bt_memcpy_d2h = _sig("bt_memcpy_d2h", [vp, vp, vp, C.c_size_t])
bt_memcpy_d2d = _sig("bt_memcpy_d2d", [vp, vp, vp, C.c_size_t])
bt_timer_create = _sig("bt_timer_create", [vp, C.POINTER(vp)])
bt_timer_destroy = _sig("bt_timer_destroy", [vp])
bt_timer_start = _sig("bt_timer_start", [vp])
bt_timer_stop = _sig("bt_timer_stop", [vp])
bt_timer_elapsed_ms = _sig("bt_timer_elapsed_ms", [vp, f32p])
bt_kmers_from_sequence = _sig("bt_kmers_from_sequence", [vp, vp, C.c_uint64, C.c_uint32, vp, vp])
bt_nthash_batch = _sig("bt_nthash_batch", [vp, vp, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, vp])
bt_bloom_create = _sig("bt_bloom_create", [vp, C.c_uint64, C.c_float, C.c_uint32, C.c_int, C.POINTER(vp)])
bt_bloom_load = _sig("bt_bloom_load", [vp, C.c_char_p, C.c_uint32, C.POINTER(vp)])
bt_bloom_save = _sig("bt_bloom_save", [vp, C.c_char_p])
bt_bloom_destroy = _sig("bt_bloom_destroy", [vp])
bt_bloom_info = _sig("bt_bloom_info", [vp, u64p, u64p, u32p, u32p, u64p])
bt_bloom_insert_batch = _sig("bt_bloom_insert_batch", [vp, vp, C.c_uint64])
bt_bloom_contains_batch = _sig("bt_bloom_contains_batch", [vp, vp, C.c_uint64, vp])
bt_bloom_read_bits = _sig("bt_bloom_read_bits", [vp, C.c_uint32, vp, C.c_uint64])
bt_bloom_clear = _sig("bt_bloom_clear", [vp])
bt_table_create = _sig("bt_table_create", [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(vp)])
bt_table_destroy = _sig("bt_table_destroy", [vp])
bt_table_status = _sig("bt_table_status", [vp, u64p, u64p, C.POINTER(C.c_int)])
bt_table_clear = _sig("bt_table_clear", [vp])
bt_table_reserve = _sig("bt_table_reserve", [vp, C.c_uint64])
bt_table_insert_batch = _sig("bt_table_insert_batch", [vp, vp, C.c_uint64, C.c_int])
bt_table_find_batch = _sig("bt_table_find_batch", [vp, vp, C.c_uint64, vp])
bt_table_read_slots = _sig("bt_table_read_slots", [vp, vp, C.c_uint64, vp, vp])
bt_table_export = _sig("bt_table_export", [vp, vp, vp, vp, C.c_uint64, u64p])
bt_table_count_row_bytes = _sig("bt_table_count_row_bytes", [vp, u32p])
bt_table_export_count_rows = _sig("bt_table_export_count_rows", [vp, vp, C.c_uint64, u64p])
bt_table_merge_count_rows = _sig("bt_table_merge_count_rows", [vp, vp, C.c_uint64])
bt_table_record_bytes = _sig("bt_table_record_bytes", [vp, u32p])
bt_table_pack = _sig("bt_table_pack", [vp, vp, C.c_uint64, u64p])
bt_table_unpack = _sig("bt_table_unpack", [vp, vp, C.c_uint64])
bt_table_save = _sig("bt_table_save", [vp, C.c_char_p, C.c_char_p])
bt_table_load = _sig("bt_table_load", [vp, C.c_char_p, C.c_char_p, C.POINTER(vp)])
bt_table_file_info = _sig("bt_table_file_info", [C.c_char_p, u32p, u32p, u64p, C.c_char_p, C.c_size_t])
bt_find_paths_create = _sig("bt_find_paths_create", [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)])
bt_find_paths_destroy = _sig("bt_find_paths_destroy", [vp])
bt_find_paths_sample = _sig("bt_find_paths_sample", [vp, vp, vp])
bt_find_paths_samples = _sig("bt_find_paths_samples", [vp, C.POINTER(vp), C.c_uint32, vp])
bt_find_paths_batch_bytes = _sig("bt_find_paths_batch_bytes", [vp, C.c_uint32, u64p])
bt_find_paths_batch_info = _sig("bt_find_paths_batch_info", [vp, C.POINTER(C.c_uint32), u64p])
bt_find_paths_sizes = _sig("bt_find_paths_sizes", [vp, vp, u64p])
bt_find_paths_fetch = _sig("bt_find_paths_fetch", [vp, vp])
bt_find_paths_info = _sig("bt_find_paths_info", [vp, vp])
bt_paths_create = _sig("bt_paths_create", [vp, vp, C.c_uint32, C.POINTER(vp), u64p])
bt_paths_destroy = _sig("bt_paths_destroy", [vp])
bt_paths_count_kmers = _sig("bt_paths_count_kmers", [vp, vp])
bt_paths_count_multigroup = _sig("bt_paths_count_multigroup", [vp, vp, vp, vp, u64p])
bt_paths_classify = _sig("bt_paths_classify", [vp, vp, vp, vp, vp])
bt_paths_candidates = _sig("bt_paths_candidates", [vp, vp, vp])
bt_paths_candidates_fetch = _sig("bt_paths_candidates_fetch", [vp, vp])
bt_paths_candidates_device = _sig("bt_paths_candidates_device", [vp, vp, vp])
bt_paths_candidates_fetch_small = _sig("bt_paths_candidates_fetch_small", [vp, vp])
bt_table_count_parameter_kmers = _sig("bt_table_count_parameter_kmers", [vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_float])
bt_table_kmer_stats = _sig("bt_table_kmer_stats", [vp, vp, vp, vp, vp, vp, vp])
bt_table_count_intercluster = _sig("bt_table_count_intercluster", [vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32])
bt_table_count_intercluster_regions = _sig("bt_table_count_intercluster_regions", [vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp])
bt_table_classify_batch = _sig("bt_table_classify_batch", [vp, vp, vp, vp, C.c_uint64, vp])
bt_kmc_scan_create = _sig("bt_kmc_scan_create", [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp, C.POINTER(vp)])
bt_kmc_scan_create_bins = _sig("bt_kmc_scan_create_bins", [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp, C.c_uint64, C.POINTER(vp)])
bt_kmc_scan_make_bloom = _sig("bt_kmc_scan_make_bloom", [vp, vp, vp, C.c_uint64, C.c_uint64])
bt_kmc_scan_destroy = _sig("bt_kmc_scan_destroy", [vp])
bt_kmc_scan_set_count_range = _sig("bt_kmc_scan_set_count_range", [vp, C.c_uint32, C.c_uint64])
bt_kmc_scan_run = _sig("bt_kmc_scan_run", [vp, vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64, vp])
bt_kmc_scan_run_host = _sig("bt_kmc_scan_run_host", [vp, vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp])
bt_kmc_scan_run_file = _sig("bt_kmc_scan_run_file", [vp, vp, vp, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp])
bt_kmc_scan_decode = _sig("bt_kmc_scan_decode", [vp, vp, C.c_uint64, C.c_uint64, vp, vp])
bt_kmer_stats_num_bins = _sig("bt_kmer_stats_num_bins", [C.c_uint32], C.c_uint64)
bt_kmc_scan_kmer_stats = _sig("bt_kmc_scan_kmer_stats", [vp, vp, C.c_uint64, C.c_uint64, vp, vp])
KMER_STATS_PROGRESS = C.CFUNCTYPE(None, C.c_uint64, vp)
bt_kmc_scan_kmer_stats_file = _sig("bt_kmc_scan_kmer_stats_file", [vp, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, u64p, u64p,
                                                                   KMER_STATS_PROGRESS, vp])
bt_reads_count = _sig("bt_reads_count", [vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp])
bt_reads_make_bloom = _sig("bt_reads_make_bloom", [vp, vp, vp, C.c_uint64, C.c_uint32])
bt_reads_sketch = _sig("bt_reads_sketch", [vp, vp, C.c_uint64, C.c_uint32, vp])
bt_reads_count_host = _sig("bt_reads_count_host", [vp, vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64, u64p])
bt_reads_make_bloom_host = _sig("bt_reads_make_bloom_host", [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint64])
bt_reads_sketch_host = _sig("bt_reads_sketch_host", [vp, vp, C.c_uint64, C.c_uint32, C.c_uint64, vp])
bt_reads_sketch_estimate = _sig("bt_reads_sketch_estimate", [vp, f64p])
bt_diag_reads_kmers = _sig("bt_diag_reads_kmers", [vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint64, u64p])
bt_diag_reads_sketch = _sig("bt_diag_reads_sketch", [vp, C.c_uint64, C.c_uint32, vp])
SKETCH_REGISTERS = 1 << 16


class BtError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise BtError(bt_last_error().decode())


def _np_ptr(a):
    return a.ctypes.data_as(vp)


class DeviceBuffer:
    """A device allocation owned by a Ctx (bt_malloc / bt_free)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = vp()
        check(bt_malloc(ctx.h, max(self.nbytes, 16), C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(bt_memcpy_h2d(self.ctx.h, self.ptr, _np_ptr(arr), arr.nbytes))
        return self

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(bt_memcpy_d2h(self.ctx.h, _np_ptr(out), self.ptr, out.nbytes))
        return out

    def zero(self):
        check(bt_memset(self.ctx.h, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self.ptr:
            bt_free(self.ctx.h, self.ptr)
            self.ptr = None


class Ctx:
    def __init__(self, device=0):
        h = vp()
        check(bt_ctx_create(device, C.byref(h)))
        self.h = h.value

    def clone(self):
        """bt_ctx_clone: a second context on the same GPU whose stream runs concurrently with this one's"""
        h = vp()
        check(bt_ctx_clone(self.h, C.byref(h)))
        c = Ctx.__new__(Ctx)
        c.h = h.value
        return c

    def sync(self):
        check(bt_sync(self.h))

    def set_stream(self, stream_ptr):
        """hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream); 0 = the device's default stream"""
        if not stream_ptr:
            check(bt_ctx_use_default_stream(self.h))
        else:
            check(bt_ctx_set_stream(self.h, stream_ptr))

    def info(self):
        cu, tot, free = C.c_int(), C.c_uint64(), C.c_uint64()
        arch = C.create_string_buffer(64)
        check(bt_ctx_info(self.h, C.byref(cu), C.byref(tot), C.byref(free), arch, 64))
        return {"num_cu": cu.value, "hbm_total": tot.value, "hbm_free": free.value, "arch": arch.value.decode()}

    def buffer(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    def close(self):
        if self.h:
            bt_ctx_destroy(self.h)
            self.h = None


class Timer:
    def __init__(self, ctx):
        h = vp()
        check(bt_timer_create(ctx.h, C.byref(h)))
        self.h = h.value

    def start(self):
        check(bt_timer_start(self.h))

    def stop(self):
        check(bt_timer_stop(self.h))

    def elapsed_ms(self):
        ms = C.c_float()
        check(bt_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        bt_timer_destroy(self.h)


class Bloom:
    """KmerBloom<k> (threaded=False) or ThreadedKmerBloom<k> (threaded=True) in HBM."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @classmethod
    def create(cls, ctx, num_kmers, fpr, k, threaded):
        h = vp()
        check(bt_bloom_create(ctx.h, num_kmers, fpr, k, int(threaded), C.byref(h)))
        return cls(ctx, h.value)

    @classmethod
    def load(cls, ctx, prefix, k):
        h = vp()
        check(bt_bloom_load(ctx.h, prefix.encode(), k, C.byref(h)))
        return cls(ctx, h.value)

    def save(self, prefix):
        check(bt_bloom_save(self.h, prefix.encode()))

    def info(self):
        nk, nb, db = C.c_uint64(), C.c_uint64(), C.c_uint64()
        nh, ns = C.c_uint32(), C.c_uint32()
        check(bt_bloom_info(self.h, C.byref(nk), C.byref(nb), C.byref(nh), C.byref(ns), C.byref(db)))
        return {"num_kmers": nk.value, "num_bits": nb.value, "num_hashes": nh.value, "num_sub": ns.value, "device_bytes": db.value}

    def insert(self, packed):
        """packed: (n, 2) uint64 host array of canonical k-mers"""
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        d = self.ctx.to_device(packed)
        check(bt_bloom_insert_batch(self.h, d.ptr, len(packed)))
        self.ctx.sync()
        d.free()

    def contains(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        n = len(packed)
        d = self.ctx.to_device(packed)
        o = self.ctx.buffer(max(n, 1))
        check(bt_bloom_contains_batch(self.h, d.ptr, n, o.ptr))
        self.ctx.sync()
        out = o.download(np.uint8, n)
        d.free()
        o.free()
        return out

    def bits(self, sub=0):
        nbytes = (self.info()["num_bits"] + 7) // 8
        out = np.empty(nbytes, dtype=np.uint8)
        check(bt_bloom_read_bits(self.h, sub, _np_ptr(out), nbytes))
        return out

    def close(self):
        if self.h:
            bt_bloom_destroy(self.h)
            self.h = None


class Table:
    """ObservedKmerCountsHash<N> in HBM."""

    def __init__(self, ctx, expected, num_samples, k):
        self.ctx, self.num_samples, self.k = ctx, num_samples, k
        h = vp()
        check(bt_table_create(ctx.h, expected, num_samples, k, C.byref(h)))
        self.h = h.value

    def status(self):
        nk, cap, ov = C.c_uint64(), C.c_uint64(), C.c_int()
        check(bt_table_status(self.h, C.byref(nk), C.byref(cap), C.byref(ov)))
        return {"num_keys": nk.value, "capacity": cap.value, "overflowed": bool(ov.value)}

    def clear(self):
        check(bt_table_clear(self.h))

    def reserve(self, expected):
        check(bt_table_reserve(self.h, expected))

    def insert(self, packed, mark_parameter=False):
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        d = self.ctx.to_device(packed)
        check(bt_table_insert_batch(self.h, d.ptr, len(packed), int(mark_parameter)))
        self.ctx.sync()
        d.free()

    def find(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        n = len(packed)
        d = self.ctx.to_device(packed)
        o = self.ctx.buffer(8 * max(n, 1))
        check(bt_table_find_batch(self.h, d.ptr, n, o.ptr))
        self.ctx.sync()
        out = o.download(np.int64, n)
        d.free()
        o.free()
        return out

    def count_intercluster(self, bloom, seq_bytes, is_decoy, female_ploidy, male_ploidy):
        arr = np.frombuffer(seq_bytes, dtype=np.uint8)
        d = self.ctx.to_device(arr)
        check(bt_table_count_intercluster(self.h, bloom.h, d.ptr, len(arr), int(is_decoy), female_ploidy, male_ploidy))
        self.ctx.sync()
        d.free()

    def count_intercluster_regions(self, bloom, seq_bytes, starts, lens, decoy, female, male):
        """bt_table_count_intercluster_regions: every region of one sequence (uploaded here) in one launch"""
        d = self.ctx.to_device(np.frombuffer(seq_bytes, dtype=np.uint8))
        a = [np.ascontiguousarray(starts, np.uint64), np.ascontiguousarray(lens, np.uint64)] + [np.ascontiguousarray(x, np.uint8) for x in (decoy, female, male)]
        assert all(len(x) == len(a[0]) for x in a)
        try:
            check(bt_table_count_intercluster_regions(self.h, bloom.h, d.ptr, len(a[0]), *[_np_ptr(x) for x in a]))
        finally:
            d.free()

    def classify(self, mg_bloom, packed, mult):
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        mult = np.ascontiguousarray(mult, dtype=np.uint8)
        n = len(packed)
        d, m = self.ctx.to_device(packed), self.ctx.to_device(mult)
        o = self.ctx.buffer(max(n, 1))
        check(bt_table_classify_batch(self.h, mg_bloom.h, d.ptr, m.ptr, n, o.ptr))
        self.ctx.sync()
        out = o.download(np.uint8, n)
        for b in (d, m, o):
            b.free()
        return out

    def count_parameter_kmers(self, bloom, seq_bytes, starts, lens, decoy, seeds, fraction):
        """bt_table_count_parameter_kmers over regions of one sequence (uploaded here)"""
        d = self.ctx.to_device(np.frombuffer(seq_bytes, dtype=np.uint8))
        a = [np.ascontiguousarray(starts, np.uint64), np.ascontiguousarray(lens, np.uint64), np.ascontiguousarray(decoy, np.uint8), np.ascontiguousarray(seeds, np.uint32)]
        check(bt_table_count_parameter_kmers(self.h, bloom.h, d.ptr, len(a[0]), *[_np_ptr(x) for x in a], float(fraction)))
        self.ctx.sync()
        d.free()

    def kmer_stats(self, gender):
        """bt_table_kmer_stats -> (class_counts[7], dict of exact integer moments n / nonzero / sum / sumsq, each [S, 256])"""
        g = np.ascontiguousarray(gender, dtype=np.uint8)
        cls = np.zeros(7, np.uint64)
        mom = {k: np.zeros((self.num_samples, 256), np.uint64) for k in ("n", "nonzero", "sum", "sumsq")}
        check(bt_table_kmer_stats(self.h, _np_ptr(g), _np_ptr(cls), _np_ptr(mom["n"]), _np_ptr(mom["nonzero"]), _np_ptr(mom["sum"]), _np_ptr(mom["sumsq"])))
        return cls, mom

    def export(self):
        """-> (kmers (n,2) u64, counts (n,S) u8, meta (n,4) u8) sorted by (hi, lo)"""
        st = self.status()
        n = st["num_keys"]
        kmers = np.zeros((max(n, 1), 2), dtype=np.uint64)
        counts = np.zeros((max(n, 1), self.num_samples), dtype=np.uint8)
        meta = np.zeros((max(n, 1), 4), dtype=np.uint8)
        w = C.c_uint64()
        check(bt_table_export(self.h, _np_ptr(kmers), _np_ptr(counts), _np_ptr(meta), max(n, 1), C.byref(w)))
        n = w.value
        return kmers[:n], counts[:n], meta[:n]

    def read_slots(self, slots):
        """bt_table_read_slots of slots found with find() -> (counts (n,S) u8, meta (n,4) u8); a slot outside the table reads as zeros"""
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        n = len(slots)
        counts = np.zeros((max(n, 1), self.num_samples), np.uint8)
        meta = np.zeros((max(n, 1), 4), np.uint8)
        check(bt_table_read_slots(self.h, _np_ptr(slots), n, _np_ptr(counts), _np_ptr(meta)))
        return counts[:n], meta[:n]

    def count_row_bytes(self):
        """bytes of a count row: 16 key + the counts padded to a multiple of four"""
        rb = C.c_uint32()
        check(bt_table_count_row_bytes(self.h, C.byref(rb)))
        return rb.value

    def export_count_rows(self):
        """bt_table_export_count_rows -> (DeviceBuffer of count rows, number of rows); the caller frees the buffer"""
        n = C.c_uint64()
        check(bt_table_export_count_rows(self.h, None, 0, C.byref(n)))
        buf = self.ctx.buffer(max(n.value, 1) * self.count_row_bytes())
        try:
            check(bt_table_export_count_rows(self.h, buf.ptr, max(n.value, 1), C.byref(n)))
        except BtError:
            buf.free()
            raise
        return buf, n.value

    def merge_count_rows(self, buf_or_ptr, n):
        """bt_table_merge_count_rows of n count rows in device memory (a DeviceBuffer or a device address); asynchronous"""
        if isinstance(buf_or_ptr, DeviceBuffer):
            assert int(n) * self.count_row_bytes() <= buf_or_ptr.nbytes
            buf_or_ptr = buf_or_ptr.ptr
        check(bt_table_merge_count_rows(self.h, buf_or_ptr, int(n)))

    def record_bytes(self):
        """bytes of a packed record: 16 key + 4 meta + the counts padded to a multiple of four"""
        rb = C.c_uint32()
        check(bt_table_record_bytes(self.h, C.byref(rb)))
        return rb.value

    def pack(self):
        """bt_table_pack -> (DeviceBuffer of packed records, number of records); the caller frees the buffer"""
        n = C.c_uint64()
        check(bt_table_pack(self.h, None, 0, C.byref(n)))
        buf = self.ctx.buffer(max(n.value, 1) * self.record_bytes())
        try:
            check(bt_table_pack(self.h, buf.ptr, max(n.value, 1), C.byref(n)))
        except BtError:
            buf.free()
            raise
        return buf, n.value

    def unpack(self, buf, n):
        """bt_table_unpack of the first n packed records of a DeviceBuffer: their meta bytes and counts are set, a key already present is an error"""
        assert int(n) * self.record_bytes() <= buf.nbytes
        check(bt_table_unpack(self.h, buf.ptr, int(n)))

    def save(self, path, manifest=""):
        check(bt_table_save(self.h, os.fsencode(path), manifest.encode()))

    @classmethod
    def load(cls, ctx, path, manifest=None):
        """bt_table_load: a new table from a checkpoint file; manifest (when given) must equal the file's"""
        h = vp()
        check(bt_table_load(ctx.h, os.fsencode(path), None if manifest is None else manifest.encode(), C.byref(h)))
        info = table_file_info(path)
        t = cls.__new__(cls)
        t.ctx, t.num_samples, t.k, t.h = ctx, info["num_samples"], info["k"], h.value
        return t

    def close(self):
        if self.h:
            bt_table_destroy(self.h)
            self.h = None


def table_file_info(path):
    """bt_table_file_info (no GPU): the verified header of a table checkpoint -> {"k", "num_samples", "num_records", "manifest"}"""
    k, ns, n = C.c_uint32(), C.c_uint32(), C.c_uint64()
    size = 1 << 16
    while True:
        text = C.create_string_buffer(size)
        check(bt_table_file_info(os.fsencode(path), C.byref(k), C.byref(ns), C.byref(n), text, size))
        if len(text.value) < size - 1 or size > 1 << 24:
            return {"k": k.value, "num_samples": ns.value, "num_records": n.value, "manifest": text.value.decode()}
        size = (1 << 24) + 1


CAND_FIELDS = [("kmer_off", np.uint32), ("hap_kmer_mult", np.uint8), ("kmer_key", np.uint64), ("kmer_has_counts", np.uint8), ("kmer_counts", np.uint8),
               ("kmer_ic_mult", np.uint8), ("kv_off", np.uint32), ("kv_var", np.uint16), ("kv_bits", np.uint32), ("unique_off", np.uint32),
               ("unique_idx", np.uint32), ("multi_off", np.uint32), ("multi_idx", np.uint32), ("hap_allele", np.uint16), ("hapnest_off", np.uint32),
               ("hapnest_idx", np.uint32), ("nestdep_off", np.uint32), ("nestdep_cluster", np.uint32), ("nestdep_var_off", np.uint32), ("nestdep_var", np.uint16)]


class _CandOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _ in CAND_FIELDS]


class _CandSizes(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rows", "mult_bytes", "nnz", "kv_words", "num_unique", "num_multi", "hap_allele", "num_haplotypes", "hapnest",
                                          "nestdep", "nestdep_var")]


class Paths:
    """Path k-mer enumeration over flattened variant-cluster graphs (bt_paths_*; input: synth_graphs.flatten-style dict)"""

    def __init__(self, ctx, flat, k):
        from . import synth_graphs

        self.ctx, self.C, self.k = ctx, flat["num_clusters"], k
        batch, self._keep = synth_graphs.to_ctypes(flat)
        h, n = vp(), C.c_uint64()
        check(bt_paths_create(ctx.h, C.byref(batch), k, C.byref(h), C.byref(n)))
        self.h, self.num_windows = h.value, n.value

    def count_kmers(self, bloom):
        check(bt_paths_count_kmers(self.h, bloom.h))

    def count_multigroup(self, cluster_group, bloom, table):
        cg = np.ascontiguousarray(cluster_group, np.uint32)
        n = C.c_uint64()
        check(bt_paths_count_multigroup(self.h, _np_ptr(cg), bloom.h, table.h, C.byref(n)))
        return n.value

    def multigroup_info(self):
        """how the last count_multigroup call ordered its groups (bt_paths_multigroup_info; the switch is BT_MG_WIDE_MIN)"""
        st = MultigroupStats()
        check(bt_paths_multigroup_info(self.h, C.byref(st)))
        return st.as_dict()

    def classify(self, table, mg_bloom):
        n = np.zeros(self.C, np.uint32)
        ex = np.zeros(self.C, np.uint8)
        check(bt_paths_classify(self.h, table.h, mg_bloom.h, _np_ptr(n), _np_ptr(ex)))
        return n, ex

    def candidates(self, table):
        sz = _CandSizes()
        check(bt_paths_candidates(self.h, table.h, C.byref(sz)))
        S = table.num_samples
        n = {"kmer_off": self.C + 1, "hap_kmer_mult": sz.mult_bytes, "kmer_key": sz.rows * 2, "kmer_has_counts": sz.rows, "kmer_counts": sz.rows * S,
             "kmer_ic_mult": sz.rows * 2, "kv_off": sz.rows + 1, "kv_var": sz.nnz, "kv_bits": sz.kv_words, "unique_off": self.C + 1, "unique_idx": sz.num_unique,
             "multi_off": self.C + 1, "multi_idx": sz.num_multi, "hap_allele": sz.hap_allele, "hapnest_off": sz.num_haplotypes + 1, "hapnest_idx": sz.hapnest,
             "nestdep_off": self.C + 1, "nestdep_cluster": sz.nestdep, "nestdep_var_off": sz.nestdep + 1, "nestdep_var": sz.nestdep_var}
        arrs = {name: np.zeros(max(int(n[name]), 1), dt) for name, dt in CAND_FIELDS}
        out = _CandOut()
        for name, _ in CAND_FIELDS:
            setattr(out, name, arrs[name].ctypes.data)
        check(bt_paths_candidates_fetch(self.h, C.byref(out)))
        return {name: arrs[name][: int(n[name])] for name, _ in CAND_FIELDS}

    _SMALL = ("kmer_off", "unique_off", "multi_off", "hap_allele", "hapnest_off", "hapnest_idx", "nestdep_off", "nestdep_cluster", "nestdep_var_off", "nestdep_var")

    def candidates_device(self, table):
        """bt_paths_candidates_device + bt_paths_candidates_fetch_small: the per-row arrays stay in device memory (GibbsSource.from_paths takes them);
        -> (sizes as a dict, the small host arrays as a dict)"""
        sz = _CandSizes()
        check(bt_paths_candidates_device(self.h, table.h, C.byref(sz)))
        self.num_samples = table.num_samples
        sizes = {n: int(getattr(sz, n)) for n, _ in _CandSizes._fields_}
        return sizes, self.fetch_small(sizes)

    def fetch_small(self, sizes):
        n = {"kmer_off": self.C + 1, "unique_off": self.C + 1, "multi_off": self.C + 1, "hap_allele": sizes["hap_allele"], "hapnest_off": sizes["num_haplotypes"] + 1,
             "hapnest_idx": sizes["hapnest"], "nestdep_off": self.C + 1, "nestdep_cluster": sizes["nestdep"], "nestdep_var_off": sizes["nestdep"] + 1,
             "nestdep_var": sizes["nestdep_var"]}
        dt = dict(CAND_FIELDS)
        arrs = {name: np.zeros(max(int(n[name]), 1), dt[name]) for name in self._SMALL}
        out = _CandOut()
        for name in self._SMALL:
            setattr(out, name, arrs[name].ctypes.data)
        check(bt_paths_candidates_fetch_small(self.h, C.byref(out)))
        return {name: arrs[name][: int(n[name])] for name in self._SMALL}

    def close(self):
        if self.h:
            bt_paths_destroy(self.h)
            self.h = None


class FindPathsStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("num_clusters", "num_wave_clusters", "wave_min_vertices", "max_vertices", "max_candidate_paths")]


class FindPaths:
    """Per-sample best-path search over flattened graphs (bt_find_paths_*)"""

    def __init__(self, ctx, flat, k, max_haps, num_samples):
        from . import synth_graphs

        self.ctx, self.C = ctx, flat["num_clusters"]
        self.nv = (flat["vertex_off"][1:] - flat["vertex_off"][:-1]).astype(np.int64)
        batch, self._keep = synth_graphs.to_ctypes(flat)
        h = vp()
        check(bt_find_paths_create(ctx.h, C.byref(batch), k, max_haps, num_samples, C.byref(h)))
        self.h = h.value

    def sample(self, bloom, seeds):
        sd = np.ascontiguousarray(seeds, np.uint32)
        check(bt_find_paths_sample(self.h, bloom.h, _np_ptr(sd)))

    def samples(self, blooms, seeds):
        """several samples in one call (bt_find_paths_samples): equal to sample() per entry, in order; seeds [n, C], a None entry is passed as a null filter"""
        n = len(blooms)
        sd = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        if sd.size != n * self.C:
            raise ValueError("seeds must hold n x num_clusters values")
        hs = (vp * max(n, 1))(*[None if b is None else b.h for b in blooms])
        check(bt_find_paths_samples(self.h, hs, n, _np_ptr(sd)))

    def batch_bytes(self, n):
        """device bytes samples() with n filters would allocate beyond what the object holds"""
        out = C.c_uint64()
        check(bt_find_paths_batch_bytes(self.h, n, C.byref(out)))
        return out.value

    def batch_info(self):
        """(largest n a samples() call had, device bytes held for batches)"""
        n, b = C.c_uint32(), C.c_uint64()
        check(bt_find_paths_batch_info(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def best_paths(self):
        n = np.zeros(self.C, np.uint32)
        tot = C.c_uint64()
        check(bt_find_paths_sizes(self.h, _np_ptr(n), C.byref(tot)))
        out = np.zeros(max(tot.value, 1), np.uint8)
        check(bt_find_paths_fetch(self.h, _np_ptr(out)))
        res, at = [], 0
        for c in range(self.C):
            m = int(n[c]) * int(self.nv[c])
            res.append(out[at:at + m].reshape(int(n[c]), int(self.nv[c])).copy())
            at += m
        return res

    def info(self):
        """how the clusters are routed (bt_find_paths_stats): num_clusters, num_wave_clusters, wave_min_vertices, max_vertices, max_candidate_paths"""
        st = FindPathsStats()
        check(bt_find_paths_info(self.h, C.byref(st)))
        return st

    def close(self):
        if self.h:
            bt_find_paths_destroy(self.h)
            self.h = None


class KmcScan:
    def __init__(self, ctx, k, p, counter_size, total, lut):
        self.ctx = ctx
        self.k, self.p, self.counter_size, self.total = k, p, counter_size, total
        self.rec_size = (k - p) // 4 + counter_size
        lut = np.ascontiguousarray(lut, dtype=np.uint64)
        h = vp()
        check(bt_kmc_scan_create_bins(ctx.h, k, p, counter_size, total, _np_ptr(lut), len(lut), C.byref(h)))   # len: 4^p + 1, or bins * 4^p + 1 (KMC2)
        self.h = h.value

    def set_count_range(self, min_count, max_count):
        check(bt_kmc_scan_set_count_range(self.h, min_count, max_count))

    def make_bloom(self, bloom, d_records_ptr, first_record, n):
        check(bt_kmc_scan_make_bloom(self.h, bloom.h, d_records_ptr, first_record, n))

    def run(self, bloom, table, sample_idx, d_records_ptr, first_record, n, d_hits_ptr=None):
        check(bt_kmc_scan_run(self.h, bloom.h, table.h, sample_idx, d_records_ptr, first_record, n, d_hits_ptr))

    def run_file(self, bloom, table, sample_idx, suf_path, first_record, n, chunk_records=0, payload_offset=4):
        """bt_kmc_scan_run_file: records [first_record, first_record + n) streamed from the .kmc_suf file -> Bloom hits (blocking)"""
        hits = C.c_uint64()
        check(bt_kmc_scan_run_file(self.h, bloom.h, table.h, sample_idx, os.fsencode(suf_path), payload_offset, first_record, n, chunk_records, C.byref(hits)))
        return hits.value

    def run_host(self, bloom, table, sample_idx, records, first_record, n, chunk_records=0):
        """bt_kmc_scan_run_host: `records` (uint8 host array) starts at record first_record -> Bloom hits (blocking)"""
        records = np.ascontiguousarray(records, dtype=np.uint8)
        assert records.nbytes >= int(n) * self.rec_size
        hits = C.c_uint64()
        check(bt_kmc_scan_run_host(self.h, bloom.h, table.h, sample_idx, _np_ptr(records), first_record, n, chunk_records, C.byref(hits)))
        return hits.value

    def decode(self, payload, first_record, n):
        d = self.ctx.to_device(np.frombuffer(payload, dtype=np.uint8))
        ok = self.ctx.buffer(16 * max(n, 1))
        oc = self.ctx.buffer(4 * max(n, 1))
        check(bt_kmc_scan_decode(self.h, d.ptr, first_record, n, ok.ptr, oc.ptr))
        self.ctx.sync()
        kmers = ok.download(np.uint64, 2 * n).reshape(n, 2)
        counts = oc.download(np.uint32, n)
        for b in (d, ok, oc):
            b.free()
        return kmers, counts

    def kmer_stats(self, d_records_ptr, first_record, n, d_hist_ptr, d_over255_ptr):
        """getKmerStats on device-resident records: ADDS into a caller-zeroed device histogram (kmer_stats_bins(k) uint64) and the device
        uint64 above-255 counter (asynchronous)"""
        check(bt_kmc_scan_kmer_stats(self.h, d_records_ptr, first_record, n, d_hist_ptr, d_over255_ptr))

    def kmer_stats_file(self, suf_path, first_record=0, n=None, chunk_records=0, payload_offset=4, progress=None):
        """getKmerStats streamed from the .kmc_suf file -> (histogram, records binned, records in range above 255); progress(records_done)
        is called after each chunk"""
        n = self.total - first_record if n is None else n
        hist = np.zeros(kmer_stats_bins(self.k), np.uint64)
        binned, over = C.c_uint64(), C.c_uint64()
        cb = KMER_STATS_PROGRESS((lambda done, _user: progress(done)) if progress else 0)
        check(bt_kmc_scan_kmer_stats_file(self.h, suf_path.encode(), payload_offset, first_record, n, chunk_records, _np_ptr(hist), C.byref(binned),
                                          C.byref(over), cb, None))
        return hist, binned.value, over.value

    def close(self):
        if self.h:
            bt_kmc_scan_destroy(self.h)
            self.h = None


def _reads_text(text):
    """a reads text (bytes, or a uint8 array) as a contiguous uint8 array"""
    return np.ascontiguousarray(np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else text, dtype=np.uint8)


def reads_count(ctx, bloom, table, sample_idx, text, host=False, chunk_bytes=0):
    """bt_reads_count (text uploaded here) or, host=True, bt_reads_count_host (text streamed through the staging slots): every k-mer occurrence of the
    reads text that hits the path filter is added to the table and to the sample's count -> occurrences that hit"""
    a = _reads_text(text)
    if host:
        hits = C.c_uint64()
        check(bt_reads_count_host(ctx.h, bloom.h, table.h, sample_idx, _np_ptr(a) if a.size else None, a.size, chunk_bytes, C.byref(hits)))
        return hits.value
    d, h = ctx.to_device(a) if a.size else None, ctx.buffer(8).zero()
    try:
        check(bt_reads_count(ctx.h, bloom.h, table.h, sample_idx, d.ptr if d else None, a.size, h.ptr))
        ctx.sync()
        return int(h.download(np.uint64, 1)[0])
    finally:
        h.free()
        if d:
            d.free()


def reads_make_bloom(ctx, bloom, text, k, host=False, chunk_bytes=0):
    """bt_reads_make_bloom / bt_reads_make_bloom_host: the k-mers of the reads text are added to a sample's filter"""
    a = _reads_text(text)
    if host:
        check(bt_reads_make_bloom_host(ctx.h, bloom.h, _np_ptr(a) if a.size else None, a.size, k, chunk_bytes))
        return
    d = ctx.to_device(a) if a.size else None
    try:
        check(bt_reads_make_bloom(ctx.h, bloom.h, d.ptr if d else None, a.size, k))
        ctx.sync()
    finally:
        if d:
            d.free()


def reads_sketch(ctx, text, k, registers=None, host=False, chunk_bytes=0):
    """bt_reads_sketch / bt_reads_sketch_host: the sketch registers (SKETCH_REGISTERS uint8; `registers`: those of earlier texts, merged into) -> registers"""
    a = _reads_text(text)
    reg = np.zeros(SKETCH_REGISTERS, np.uint8) if registers is None else np.array(registers, dtype=np.uint8)
    assert reg.size == SKETCH_REGISTERS
    if host:
        check(bt_reads_sketch_host(ctx.h, _np_ptr(a) if a.size else None, a.size, k, chunk_bytes, _np_ptr(reg)))
        return reg
    d, r = ctx.to_device(a) if a.size else None, ctx.to_device(reg)
    try:
        check(bt_reads_sketch(ctx.h, d.ptr if d else None, a.size, k, r.ptr))
        ctx.sync()
        return r.download(np.uint8, SKETCH_REGISTERS)
    finally:
        r.free()
        if d:
            d.free()


def reads_sketch_estimate(registers):
    """bt_reads_sketch_estimate (no GPU): the number of distinct k-mers a sketch has seen"""
    reg = np.ascontiguousarray(registers, dtype=np.uint8)
    assert reg.size == SKETCH_REGISTERS
    out = C.c_double()
    check(bt_reads_sketch_estimate(_np_ptr(reg), C.byref(out)))
    return out.value


def diag_reads_sketch(text, k, registers=None):
    """bt_diag_reads_sketch (no GPU): the sketch registers of a reads text from the kernels' window code run on the host"""
    a = _reads_text(text)
    reg = np.zeros(SKETCH_REGISTERS, np.uint8) if registers is None else np.array(registers, dtype=np.uint8)
    assert reg.size == SKETCH_REGISTERS
    check(bt_diag_reads_sketch(_np_ptr(a) if a.size else None, a.size, k, _np_ptr(reg)))
    return reg


def diag_reads_kmers(text, k):
    """bt_diag_reads_kmers (no GPU): the kernels' window code run on the host -> (canonical k-mers (n, 2) uint64, hashes (n,), index of each window's last byte
    (n,)), in text order"""
    a = _reads_text(text)
    cap = max(a.size, 1)
    kmers, hashes, ends = np.zeros((cap, 2), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    n = C.c_uint64()
    check(bt_diag_reads_kmers(_np_ptr(a) if a.size else None, a.size, k, _np_ptr(kmers), _np_ptr(hashes), _np_ptr(ends), cap, C.byref(n)))
    return kmers[:n.value].copy(), hashes[:n.value].copy(), ends[:n.value].copy()


bt_reads_packed_bytes = _sig("bt_reads_packed_bytes", [C.c_uint64], C.c_uint64)
bt_reads_pack = _sig("bt_reads_pack", [vp, vp, C.c_uint64, vp])
bt_reads_unpack = _sig("bt_reads_unpack", [vp, vp, C.c_uint64, vp])
bt_diag_reads_pack = _sig("bt_diag_reads_pack", [vp, C.c_uint64, vp])
bt_diag_reads_unpack = _sig("bt_diag_reads_unpack", [vp, C.c_uint64, vp])
bt_reads_count_packed = _sig("bt_reads_count_packed", [vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp])
bt_reads_make_bloom_packed = _sig("bt_reads_make_bloom_packed", [vp, vp, vp, C.c_uint64, C.c_uint32])
bt_reads_sketch_packed = _sig("bt_reads_sketch_packed", [vp, vp, C.c_uint64, C.c_uint32, vp])
bt_reads_count_packed_host = _sig("bt_reads_count_packed_host", [vp, vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64, u64p])
bt_reads_make_bloom_packed_host = _sig("bt_reads_make_bloom_packed_host", [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint64])
bt_reads_sketch_packed_host = _sig("bt_reads_sketch_packed_host", [vp, vp, C.c_uint64, C.c_uint32, C.c_uint64, vp])
bt_diag_reads_kmers_packed = _sig("bt_diag_reads_kmers_packed", [vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint64, u64p])


class ReadsPackInfo(C.Structure):   # include/btgpu.h: bt_reads_pack_info
    _fields_ = [("version", C.c_uint32), ("k", C.c_uint32), ("block_positions", C.c_uint32), ("manifest_bytes", C.c_uint32), ("sections", C.c_uint64),
                ("positions", C.c_uint64), ("bases", C.c_uint64), ("reads", C.c_uint64), ("max_section_positions", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


bt_reads_pack_writer_create = _sig("bt_reads_pack_writer_create", [C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(vp)])
bt_reads_pack_writer_add = _sig("bt_reads_pack_writer_add", [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64])
bt_reads_pack_writer_finish = _sig("bt_reads_pack_writer_finish", [vp])
bt_reads_pack_writer_destroy = _sig("bt_reads_pack_writer_destroy", [vp], None)
bt_reads_pack_reader_open = _sig("bt_reads_pack_reader_open", [C.c_char_p, C.POINTER(vp), C.POINTER(ReadsPackInfo)])
bt_reads_pack_reader_manifest = _sig("bt_reads_pack_reader_manifest", [vp, vp, C.c_uint64, u64p])
bt_reads_pack_reader_next = _sig("bt_reads_pack_reader_next", [vp, vp, C.c_uint64, u64p, u64p, u64p, C.POINTER(C.c_int)])
bt_reads_pack_reader_close = _sig("bt_reads_pack_reader_close", [vp], None)
bt_reads_pack_file_info = _sig("bt_reads_pack_file_info", [C.c_char_p, C.POINTER(ReadsPackInfo)])


def reads_packed_bytes(positions):
    """bt_reads_packed_bytes: 48 * ceil(positions / 128)"""
    return int(bt_reads_packed_bytes(positions))


def _packed_array(packed, positions):
    """packed reads (bytes, or a uint8 array) as a contiguous, 4-byte aligned uint8 array of at least reads_packed_bytes(positions) bytes"""
    a = _reads_text(packed)
    assert a.size >= reads_packed_bytes(positions), (a.size, positions)
    if a.ctypes.data & 3:
        b = np.empty(a.size // 4 + 1, np.uint32).view(np.uint8)[:a.size]
        b[:] = a
        a = b
    return a


def diag_reads_pack(text):
    """bt_diag_reads_pack (no GPU): a reads text -> its packed form, a uint8 array of reads_packed_bytes(len(text)) bytes"""
    a = _reads_text(text)
    out = np.zeros(reads_packed_bytes(a.size) // 4, np.uint32).view(np.uint8)
    check(bt_diag_reads_pack(_np_ptr(a) if a.size else None, a.size, _np_ptr(out) if out.size else None))
    return out


def diag_reads_unpack(packed, positions):
    """bt_diag_reads_unpack (no GPU): packed reads -> the canonical text (upper-case bases, every invalid position a newline) as bytes"""
    p = _packed_array(packed, positions)
    out = np.zeros(positions, np.uint8)
    check(bt_diag_reads_unpack(_np_ptr(p) if p.size else None, positions, _np_ptr(out) if positions else None))
    return out.tobytes()


def reads_pack(ctx, text, misalign=0):
    """bt_reads_pack over a host text (uploaded `misalign` bytes into its allocation) -> the packed form as a uint8 array"""
    a = _reads_text(text)
    n = reads_packed_bytes(a.size)
    if not a.size:
        check(bt_reads_pack(ctx.h, None, 0, None))
        return np.zeros(0, np.uint8)
    d_in, d_out = ctx.buffer(a.size + misalign), ctx.buffer(n)
    try:
        check(bt_memcpy_h2d(ctx.h, d_in.ptr + misalign, _np_ptr(a), a.size))
        check(bt_memset(ctx.h, d_out.ptr, 0xA5, n))   # every word of the output is written by the kernel
        check(bt_reads_pack(ctx.h, d_in.ptr + misalign, a.size, d_out.ptr))
        ctx.sync()
        return d_out.download(np.uint8, n)
    finally:
        d_in.free()
        d_out.free()


def reads_unpack(ctx, packed, positions, misalign=0):
    """bt_reads_unpack over a host buffer -> the canonical text as bytes (written `misalign` bytes into its allocation)"""
    p = _packed_array(packed, positions)
    if not positions:
        check(bt_reads_unpack(ctx.h, None, 0, None))
        return b""
    d_in, d_out = ctx.to_device(p), ctx.buffer(positions + misalign + 16)
    try:
        check(bt_memset(ctx.h, d_out.ptr, 0x23, positions + misalign + 16))
        check(bt_reads_unpack(ctx.h, d_in.ptr, positions, d_out.ptr + misalign))
        ctx.sync()
        whole = d_out.download(np.uint8, positions + misalign + 16)
        assert (whole[:misalign] == 0x23).all() and (whole[misalign + positions:] == 0x23).all(), "bt_reads_unpack wrote outside its text"
        return whole[misalign:misalign + positions].tobytes()
    finally:
        d_in.free()
        d_out.free()


def reads_count_packed(ctx, bloom, table, sample_idx, packed, positions, host=False, chunk_bytes=0):
    """bt_reads_count_packed (packed reads uploaded here) or, host=True, bt_reads_count_packed_host -> occurrences that hit the path filter"""
    p = _packed_array(packed, positions)
    if host:
        hits = C.c_uint64()
        check(bt_reads_count_packed_host(ctx.h, bloom.h, table.h, sample_idx, _np_ptr(p) if p.size else None, positions, chunk_bytes, C.byref(hits)))
        return hits.value
    d, h = ctx.to_device(p) if p.size else None, ctx.buffer(8).zero()
    try:
        check(bt_reads_count_packed(ctx.h, bloom.h, table.h, sample_idx, d.ptr if d else None, positions, h.ptr))
        ctx.sync()
        return int(h.download(np.uint64, 1)[0])
    finally:
        h.free()
        if d:
            d.free()


def reads_make_bloom_packed(ctx, bloom, packed, positions, k, host=False, chunk_bytes=0):
    """bt_reads_make_bloom_packed / bt_reads_make_bloom_packed_host: the k-mers of the packed reads are added to a sample's filter"""
    p = _packed_array(packed, positions)
    if host:
        check(bt_reads_make_bloom_packed_host(ctx.h, bloom.h, _np_ptr(p) if p.size else None, positions, k, chunk_bytes))
        return
    d = ctx.to_device(p) if p.size else None
    try:
        check(bt_reads_make_bloom_packed(ctx.h, bloom.h, d.ptr if d else None, positions, k))
        ctx.sync()
    finally:
        if d:
            d.free()


def reads_sketch_packed(ctx, packed, positions, k, registers=None, host=False, chunk_bytes=0):
    """bt_reads_sketch_packed / bt_reads_sketch_packed_host -> the sketch registers (`registers`: those of earlier texts, merged into)"""
    p = _packed_array(packed, positions)
    reg = np.zeros(SKETCH_REGISTERS, np.uint8) if registers is None else np.array(registers, dtype=np.uint8)
    assert reg.size == SKETCH_REGISTERS
    if host:
        check(bt_reads_sketch_packed_host(ctx.h, _np_ptr(p) if p.size else None, positions, k, chunk_bytes, _np_ptr(reg)))
        return reg
    d, r = ctx.to_device(p) if p.size else None, ctx.to_device(reg)
    try:
        check(bt_reads_sketch_packed(ctx.h, d.ptr if d else None, positions, k, r.ptr))
        ctx.sync()
        return r.download(np.uint8, SKETCH_REGISTERS)
    finally:
        r.free()
        if d:
            d.free()


def diag_reads_kmers_packed(packed, positions, k):
    """bt_diag_reads_kmers_packed (no GPU): diag_reads_kmers over packed reads -> (canonical k-mers (n, 2), hashes (n,), end positions (n,))"""
    p = _packed_array(packed, positions)
    cap = max(positions, 1)
    kmers, hashes, ends = np.zeros((cap, 2), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    n = C.c_uint64()
    check(bt_diag_reads_kmers_packed(_np_ptr(p) if p.size else None, positions, k, _np_ptr(kmers), _np_ptr(hashes), _np_ptr(ends), cap, C.byref(n)))
    return kmers[:n.value].copy(), hashes[:n.value].copy(), ends[:n.value].copy()


class ReadsPackWriter:
    """bt_reads_pack_writer: a reads pack file written section by section; nothing exists under `path` until finish()"""

    def __init__(self, path, k, manifest=""):
        self.h = vp()
        check(bt_reads_pack_writer_create(os.fsencode(path), k, manifest.encode(), C.byref(self.h)))

    def add(self, packed, positions, bases, reads):
        p = _packed_array(packed, positions)
        check(bt_reads_pack_writer_add(self.h, _np_ptr(p) if p.size else None, positions, bases, reads))

    def finish(self):
        check(bt_reads_pack_writer_finish(self.h))

    def close(self):
        if self.h:
            bt_reads_pack_writer_destroy(self.h)
            self.h = None


class ReadsPackReader:
    """bt_reads_pack_reader: open() validates the header, the section heads, the trailer and the file's size; sections() reads and checks the payloads"""

    def __init__(self, path):
        self.h = vp()
        self._info = ReadsPackInfo()
        check(bt_reads_pack_reader_open(os.fsencode(path), C.byref(self.h), C.byref(self._info)))

    def info(self):
        return self._info.as_dict()

    def manifest(self):
        buf, n = np.zeros(max(self._info.manifest_bytes, 1), np.uint8), C.c_uint64()
        check(bt_reads_pack_reader_manifest(self.h, _np_ptr(buf), buf.size, C.byref(n)))
        return buf[:n.value].tobytes().decode()

    def next(self):
        """-> (packed uint8 array, positions, bases, reads), or None after the last section"""
        buf = np.zeros(max(reads_packed_bytes(self._info.max_section_positions) // 4, 1), np.uint32).view(np.uint8)
        positions, bases, reads, end = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(bt_reads_pack_reader_next(self.h, _np_ptr(buf), buf.size, C.byref(positions), C.byref(bases), C.byref(reads), C.byref(end)))
        if end.value:
            return None
        return buf[:reads_packed_bytes(positions.value)], positions.value, bases.value, reads.value

    def sections(self):
        while True:
            s = self.next()
            if s is None:
                return
            yield s

    def close(self):
        if self.h:
            bt_reads_pack_reader_close(self.h)
            self.h = None


def reads_pack_file_info(path):
    """bt_reads_pack_file_info (no GPU) -> dict of the header's and the trailer's fields; an error names the defect"""
    info = ReadsPackInfo()
    check(bt_reads_pack_file_info(os.fsencode(path), C.byref(info)))
    return info.as_dict()


def kmer_stats_bins(k):
    """bins of the getKmerStats histogram: 256 counts x C(k+3,3) compositions (include/btgpu.h)"""
    return int(bt_kmer_stats_num_bins(k))


def kmer_stats_rows(hist, k):
    """the non-zero bins of a getKmerStats histogram as rows (number, count, A, C, G, T), in bin order = sorted by (count, A, C, G, T)"""
    comp = np.array([(a, c, g, k - a - c - g) for a in range(k + 1) for c in range(k + 1 - a) for g in range(k + 1 - a - c)], np.int64)
    hist = np.asarray(hist, np.uint64)
    assert len(hist) == 256 * len(comp)
    nz = np.nonzero(hist)[0]
    count, idx = np.divmod(nz, len(comp))
    return np.column_stack([hist[nz].astype(np.int64), count, comp[idx]])


# ---------------------------------------------------------------------------------------------------------------
# Gibbs genotyping (bt_gibbs_*)
# ---------------------------------------------------------------------------------------------------------------
bt_gibbs_create = _sig("bt_gibbs_create", [vp, vp, vp, C.POINTER(vp)])
bt_gibbs_destroy = _sig("bt_gibbs_destroy", [vp])
bt_gibbs_set_lut = _sig("bt_gibbs_set_lut", [vp, vp, vp])
bt_gibbs_set_noise_lut = _sig("bt_gibbs_set_noise_lut", [vp, vp])
bt_gibbs_init_chain = _sig("bt_gibbs_init_chain", [vp, C.c_uint32])
bt_gibbs_sweep = _sig("bt_gibbs_sweep", [vp, C.c_uint32, C.c_int])
bt_gibbs_run = _sig("bt_gibbs_run", [vp])
bt_gibbs_noise_counts = _sig("bt_gibbs_noise_counts", [vp, vp, C.c_int])
bt_gibbs_noise_iteration = _sig("bt_gibbs_noise_iteration", [vp, vp, C.c_int, vp])
bt_gibbs_noise_chain_begin = _sig("bt_gibbs_noise_chain_begin", [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)])
bt_gibbs_noise_chain_step = _sig("bt_gibbs_noise_chain_step", [vp, vp, vp])
bt_gibbs_noise_chain_end = _sig("bt_gibbs_noise_chain_end", [vp])
bt_ctx_clone = _sig("bt_ctx_clone", [vp, C.POINTER(vp)])
bt_gibbs_reset_groups = _sig("bt_gibbs_reset_groups", [vp])
bt_gibbs_sparse_forms = _sig("bt_gibbs_sparse_forms", [vp, vp])
bt_gibbs_result_sizes = _sig("bt_gibbs_result_sizes", [vp, u64p, u64p])
bt_gibbs_result_fetch = _sig("bt_gibbs_result_fetch", [vp] * 7)
bt_gibbs_result_words = _sig("bt_gibbs_result_words", [vp, C.POINTER(vp), u64p])
bt_gibbs_genotypes = _sig("bt_gibbs_genotypes", [vp, vp, C.POINTER(vp), u64p])
bt_gibbs_trace_enable = _sig("bt_gibbs_trace_enable", [vp, C.c_uint32])
bt_gibbs_trace_fetch = _sig("bt_gibbs_trace_fetch", [vp, vp, C.c_uint64, u64p])
bt_gibbs_posterior_summary = _sig("bt_gibbs_posterior_summary", [vp, vp])
bt_gibbs_timeline_enable = _sig("bt_gibbs_timeline_enable", [vp, C.c_uint32])
bt_gibbs_timeline_sizes = _sig("bt_gibbs_timeline_sizes", [vp, u64p, u32p, u32p, u32p])
bt_gibbs_timeline_fetch = _sig("bt_gibbs_timeline_fetch", [vp, vp, C.c_uint64, u64p])
bt_gibbs_timeline_summary = _sig("bt_gibbs_timeline_summary", [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp])
bt_gibbs_device_bytes = _sig("bt_gibbs_device_bytes", [vp, u64p])
bt_gibbs_source_create = _sig("bt_gibbs_source_create", [vp, C.c_uint32, vp, C.POINTER(vp)])
bt_gibbs_source_create_from_paths = _sig("bt_gibbs_source_create_from_paths", [vp, C.c_uint32, vp, vp, C.POINTER(vp)])
bt_gibbs_source_fetch = _sig("bt_gibbs_source_fetch", [vp, vp, vp])
bt_gibbs_source_destroy = _sig("bt_gibbs_source_destroy", [vp])
bt_gibbs_source_device_bytes = _sig("bt_gibbs_source_device_bytes", [vp, u64p])
bt_gibbs_create_from_source = _sig("bt_gibbs_create_from_source", [vp, vp, vp, vp, C.c_uint32, C.POINTER(vp)])
bt_gibbs_state_bytes = _sig("bt_gibbs_state_bytes", [vp, vp, vp, u64p])
bt_gibbs_state_bytes_from_source = _sig("bt_gibbs_state_bytes_from_source", [vp, vp, vp, C.c_uint32, u64p])
bt_diag_uset_replay = _sig("bt_diag_uset_replay", [C.c_uint32, vp, vp, C.c_uint64, vp, u32p])
bt_diag_nset_replay = _sig("bt_diag_nset_replay", [C.c_uint32, vp, vp, C.c_uint64, vp, u32p, vp])
bt_diag_nset_max = _sig("bt_diag_nset_max", [], C.c_uint32)
bt_diag_rng = _sig("bt_diag_rng", [C.c_uint32, C.c_int, vp, vp, C.c_uint64, vp])
bt_diag_bulk_bernoulli = _sig("bt_diag_bulk_bernoulli", [C.c_uint32, C.c_uint64, C.c_uint32, C.c_double, C.c_uint32, C.c_int, vp, vp, vp])
bt_rng_probe = _sig("bt_rng_probe", [vp, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp])
bt_diag_rng_probe = _sig("bt_diag_rng_probe", [C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp])
# include/btgpu.h: bt_rng_probe_gen, bt_rng_probe_step, the step kinds and the ring places
PROBE_GEN = np.dtype([(n, np.uint32) for n in ("seed", "discard", "ring_cap", "ring_place", "step_off", "num_steps", "copies", "reserved")])
PROBE_STEP = np.dtype([("kind", np.uint32), ("n", np.uint32), ("a", np.float64), ("b", np.float64), ("c", np.float64), ("d", np.float64)])
(PROBE_DRAW, PROBE_TOPUP, PROBE_REOPEN, PROBE_CANONICAL, PROBE_CANONICAL2, PROBE_UNIFORM_INT, PROBE_BERNOULLI, PROBE_SHUFFLE, PROBE_NORMAL, PROBE_GAMMA, PROBE_BULK,
 PROBE_DIRECT, PROBE_SCREEN) = range(13)
PROBE_RING_HBM, PROBE_RING_LDS, PROBE_RING_LDS_FLAT = range(3)


def rng_probe(ctx, lane_gen, gens, steps, row_cap):
    """bt_rng_probe (ctx a Ctx) or its host twin bt_diag_rng_probe (ctx None) -> (rows [cases][64][row_cap], finals [cases][64][12]); the second index is the
    lane on the device and the generator on the host"""
    lane_gen = np.ascontiguousarray(lane_gen, np.int32).reshape(-1, 64)
    gens = np.ascontiguousarray(gens, PROBE_GEN).reshape(-1, 64)
    steps = np.ascontiguousarray(steps, PROBE_STEP).reshape(-1)
    n = lane_gen.shape[0]
    if gens.shape[0] != n:
        raise ValueError("rng_probe: one generator table per case")
    rows = np.zeros((n, 64, int(row_cap)), np.uint32)
    fin = np.zeros((n, 64, 12), np.uint32)
    args = (n, _np_ptr(lane_gen), _np_ptr(gens), _np_ptr(steps) if steps.size else None, steps.size, int(row_cap), _np_ptr(rows), _np_ptr(fin))
    check(bt_rng_probe(ctx.h, *args) if ctx is not None else bt_diag_rng_probe(*args))
    return rows, fin


bt_genotype_text_sizes = _sig("bt_genotype_text_sizes", [vp, vp, C.c_uint64, u64p, u64p])
bt_genotype_text = _sig("bt_genotype_text", [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, u32p])
bt_gibbs_genotype_text = _sig("bt_gibbs_genotype_text", [vp, vp, C.POINTER(vp), u64p, C.POINTER(vp), u64p, u32p])
bt_diag_genotype_text = _sig("bt_diag_genotype_text", [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, u32p])
bt_diag_format_g6 = _sig("bt_diag_format_g6", [vp, C.c_uint64, vp, vp])
bt_diag_genotype_cluster = _sig("bt_diag_genotype_cluster", [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p])
bt_diag_kmer_set_order = _sig("bt_diag_kmer_set_order", [vp, C.c_uint32, C.c_uint64, C.c_uint, vp, vp])
bt_diag_kmer_set_order_staged = _sig("bt_diag_kmer_set_order_staged", [vp, C.c_uint32, C.c_uint64, C.c_uint, vp, vp])
bt_diag_std_hash_bitset = _sig("bt_diag_std_hash_bitset", [C.c_uint64, C.c_uint64, C.c_uint], C.c_uint64)
bt_kmer_set_orders = _sig("bt_kmer_set_orders", [vp, vp, vp, C.c_uint32, C.c_uint, C.c_uint64, C.c_uint32, vp, vp, vp])
bt_paths_multigroup_info = _sig("bt_paths_multigroup_info", [vp, vp])


# include/btgpu.h: bt_gibbs_timeline_record (48 bytes) and bt_gibbs_timeline_summary_t
TIMELINE_RECORD = np.dtype([("start_tick", np.uint64), ("end_tick", np.uint64), ("hw_id", np.uint32), ("xcc_id", np.uint32), ("tile", np.uint32), ("wave", np.uint32),
                            ("launch", np.uint32), ("launch_class", np.uint16), ("kernel", np.uint8), ("op", np.uint8), ("groups", np.uint32), ("lds_bytes", np.uint32)])
assert TIMELINE_RECORD.itemsize == 48
TIMELINE_KERNELS = ("general", "hot", "simple", "single")   # bt_gibbs_timeline_record::kernel
_TIMELINE_SUMMARY_FIELDS = ("records", "unfinished", "first_start", "last_end", "busy_ticks", "peak_live", "median_end", "idle_after_median_ticks", "last_record")


def timeline_summary(records, launch=None, launch_class=None):
    """bt_gibbs_timeline_summary (host only, exact integer ticks) of a TIMELINE_RECORD array -> dict; last_record is None when no record is selected"""
    records = np.ascontiguousarray(records, TIMELINE_RECORD)
    out = np.zeros(len(_TIMELINE_SUMMARY_FIELDS), np.uint64)
    check(bt_gibbs_timeline_summary(_np_ptr(records) if len(records) else None, len(records), 0xFFFFFFFF if launch is None else int(launch),
                                    0xFFFFFFFF if launch_class is None else int(launch_class), _np_ptr(out)))
    d = {k: int(v) for k, v in zip(_TIMELINE_SUMMARY_FIELDS, out)}
    if d["last_record"] == 0xFFFFFFFFFFFFFFFF:
        d["last_record"] = None
    return d


class MultigroupStats(C.Structure):   # include/btgpu.h: bt_multigroup_stats
    _fields_ = [(n, C.c_uint32) for n in ("num_groups", "num_wide_groups", "wide_min_kmers", "max_group_kmers", "max_stages")] + [("wide_scratch_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def kmer_set_orders(ctx, groups, k, initial_buckets=1, wide_min=0):
    """bt_kmer_set_orders: groups = arrays [n_g, 2] of distinct packed k-mers in insertion order -> (ranks per group, bucket count after each group, stats)"""
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint64).reshape(-1, 2) for g in groups]) if len(groups) else np.zeros((0, 2), np.uint64))
    rank = np.zeros(max(int(off[-1]), 1), np.uint32)
    final = np.zeros(max(len(groups), 1), np.uint64)
    stats = MultigroupStats()
    check(bt_kmer_set_orders(ctx.h, _np_ptr(flat) if len(flat) else None, _np_ptr(off), len(groups), k, initial_buckets, wide_min, _np_ptr(rank), _np_ptr(final), C.byref(stats)))
    return [rank[int(off[g]):int(off[g + 1])] for g in range(len(groups))], final[:len(groups)], stats.as_dict()


bt_noise_model_create = _sig("bt_noise_model_create", [vp, C.c_uint32, vp, C.POINTER(vp)])
bt_noise_model_destroy = _sig("bt_noise_model_destroy", [vp])
bt_noise_model_set_rng = _sig("bt_noise_model_set_rng", [vp, vp])
bt_noise_model_get_rng = _sig("bt_noise_model_get_rng", [vp, vp])
NOISE_REDUCE = C.CFUNCTYPE(C.c_int, vp, vp, C.c_uint64)
bt_gibbs_noise_chain = _sig("bt_gibbs_noise_chain", [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp])


class NoiseRng(C.Structure):   # include/btgpu.h: bt_noise_rng
    _fields_ = [("mt", C.c_uint32 * 624), ("mt_pos", C.c_uint32), ("saved_available", C.c_uint32), ("saved", C.c_double)]


class NoiseModel:
    """the noise half of the count model on the device (bt_noise_model_*): priors [(shape, scale)] per sample + the run's generator"""

    def __init__(self, ctx, priors):
        self.ctx, self.S = ctx, len(priors)
        pr = np.ascontiguousarray(np.asarray(priors, np.float32).reshape(-1))
        h = vp()
        check(bt_noise_model_create(ctx.h, self.S, _np_ptr(pr), C.byref(h)))
        self.h = h.value

    def set_generator(self, words626, saved):
        """words626 / saved as count_model.CountDistribution.export_generator() returns them"""
        r = NoiseRng()
        C.memmove(r.mt, np.ascontiguousarray(words626[:624], np.uint32).ctypes.data, 624 * 4)
        r.mt_pos, r.saved_available, r.saved = int(words626[624]), int(words626[625]), float(saved)
        check(bt_noise_model_set_rng(self.h, C.addressof(r)))

    def get_generator(self):
        r = NoiseRng()
        check(bt_noise_model_get_rng(self.h, C.addressof(r)))
        w = np.zeros(626, np.uint32)
        w[:624] = np.frombuffer(r.mt, np.uint32)
        w[624], w[625] = r.mt_pos, r.saved_available
        return w, r.saved

    def chain(self, gibbs, num_iterations, first_collect, reduce=None):
        """bt_gibbs_noise_chain -> rates [num_iterations, S]; reduce(d_hist_ptr, n) must only enqueue work on the context's stream"""
        rates = np.zeros(num_iterations * self.S)
        cb = None
        if reduce is not None:
            def hook(_user, d_hist, n):
                try:
                    reduce(d_hist, n)
                    return 0
                except Exception:   # an exception must not unwind through the library's frames
                    return 1
            cb = NOISE_REDUCE(hook)
        check(bt_gibbs_noise_chain(gibbs.h if gibbs is not None else None, self.h, num_iterations, first_collect, C.cast(cb, vp) if cb is not None else None, None, _np_ptr(rates)))
        return rates.reshape(num_iterations, self.S)

    def close(self):
        if self.h:
            bt_noise_model_destroy(self.h)
            self.h = None


def parse_result_words(w):
    """one launch's word string (bt_gibbs_result_words) -> (the dictionary Gibbs.results() returns, words consumed)"""
    w = np.ascontiguousarray(w, np.uint32)
    Cn, nd, nc, S = (int(x) for x in w[:4])
    sizes = w[4:4 + 2 * Cn].reshape(Cn, 2).astype(np.uint64)
    at = 4 + 2 * Cn
    keys = w[at:at + nd]
    at += nd
    freq = w[at:at + nd * S].reshape(nd, S)
    at = (at + nd * S + 1) & ~1
    stats = w[at:at + nc * 24].copy().view(np.float64).reshape(nc, 3, 4)
    at += nc * 24
    dip_off = np.concatenate([[0], np.cumsum(sizes[:, 0])]).astype(np.uint64)
    cell_off = np.concatenate([[0], np.cumsum(sizes[:, 1])]).astype(np.uint64)
    return {"dip_off": dip_off, "h1": (keys & 0xFFFF).astype(np.uint16), "h2": (keys >> 16).astype(np.uint16), "freq": freq.copy(), "cell_off": cell_off, "stats": stats}, at


class GenotypeFilters(C.Structure):   # include/btgpu.h: bt_genotype_filters
    _fields_ = [("min_genotype_posterior", C.c_float), ("min_number_of_kmers", C.c_float), ("min_fraction_observed_kmers", vp)]


def _genotype_filters(min_gpp, min_kmers, min_fraction):
    mf = np.ascontiguousarray(min_fraction, np.float32)
    f = GenotypeFilters()
    f.min_genotype_posterior, f.min_number_of_kmers, f.min_fraction_observed_kmers = min_gpp, min_kmers, mf.ctypes.data
    return f, mf


_log10f = None


def genotype_quality(best):
    """GQ from the best genotype posterior as the host layer derives it (Genotypes.cpp: floatCompare against 1 and 0, else
    (uint32_t)(-10 * log10f(1 - best)) with the C library's log10f — the digit depends on its last bit, so numpy's own log10 will not do)"""
    global _log10f
    if _log10f is None:
        import ctypes.util

        m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _log10f = m.log10f
        _log10f.argtypes, _log10f.restype = [C.c_float], C.c_float
    f32 = np.float32

    def cmp(a, b):
        return a == b or abs(f32(a - b)) < f32(f32(abs(min(a, b)) * np.finfo(f32).eps) * f32(100))

    best = f32(best)
    if cmp(best, f32(1)):
        return 99
    if cmp(best, f32(0)):
        return 0
    return int(f32(f32(-10) * f32(_log10f(f32(f32(1) - best)))))


def parse_genotype_words(w):
    """one launch's genotype string (bt_gibbs_genotypes / bt_diag_genotype_cluster; layout: include/btgpu.h) -> per cluster, in the sampler's cluster
    order, the dictionary of arrays bayestyper_amd.host.genotypes.cluster_genotypes returns (gq derived from `best` on the host), plus "best" [V, S],
    "ploidy" [S] and "kmer_means" [V, S, Amax, 3] (count / fraction / mean statistic: NAK, FAK, MAC; rows past a variant's alleles are 0)"""
    w = np.ascontiguousarray(w, np.uint32)
    Cn, NV, S = int(w[0]), int(w[1]), int(w[2])
    cvo = w[4:4 + Cn + 1].astype(np.int64)
    voff = w[5 + Cn:5 + Cn + NV + 1].astype(np.int64)
    fw = w.view(np.float32)
    out = []
    for c in range(Cn):
        v0, V = int(cvo[c]), int(cvo[c + 1] - cvo[c])
        vna = np.array([w[voff[v0 + v]] for v in range(V)], np.uint16)
        Amax = int(vna.max()) if V else 0
        Gmax = Amax * (Amax + 1) // 2
        d = {"gpp": np.zeros((V, S, Gmax), np.float32), "app": np.zeros((V, S, Amax), np.float32), "filters": np.zeros((V, S, Amax), np.uint16),
             "estimate": np.full((V, S, 2), 0xFFFF, np.uint16), "gq": np.zeros((V, S), np.uint32), "total_count": np.zeros(V, np.uint32),
             "alt_counts": np.zeros((V, Amax), np.uint32), "alt_freq": np.zeros((V, Amax), np.float32), "acp": np.zeros((V, Amax), np.float32),
             "max_alt_acp": np.zeros(V, np.float32), "non_covered": np.zeros((V, Amax), np.uint8), "num_alleles": vna,
             "best": np.zeros((V, S), np.float32), "ploidy": np.zeros(S, np.uint8), "kmer_means": np.zeros((V, S, Amax, 3), np.float64),
             "has_dependency": np.zeros(V, np.uint8)}
        for v in range(V):
            at = int(voff[v0 + v])
            A = int(w[at])
            d["total_count"][v], d["max_alt_acp"][v], d["has_dependency"][v] = w[at + 1], fw[at + 2], w[at + 3]
            al = w[at + 4:at + 4 + 4 * A].reshape(A, 4)
            d["acp"][v, :A] = al[:, 0].view(np.float32)
            d["alt_counts"][v, :A - 1] = al[1:, 1]
            d["alt_freq"][v, :A - 1] = al[1:, 2].view(np.float32)
            d["non_covered"][v, :A] = al[:, 3]
            at += 4 + 4 * A
            for s in range(S):
                ploidy = int(w[at])
                d["ploidy"][s] = ploidy
                d["estimate"][v, s] = (w[at + 1] & 0xFFFF, w[at + 1] >> 16)
                d["best"][v, s] = fw[at + 2]
                d["gq"][v, s] = genotype_quality(fw[at + 2])
                G = A * (A + 1) // 2 if ploidy == 2 else (A if ploidy == 1 else 0)
                Ap = A if ploidy else 0
                d["gpp"][v, s, :G] = fw[at + 4:at + 4 + G]
                d["app"][v, s, :Ap] = fw[at + 4 + G:at + 4 + G + Ap]
                d["filters"][v, s, :Ap] = w[at + 4 + G + Ap:at + 4 + G + 2 * Ap]
                at += 4 + G + 2 * Ap
                at += at & 1
                d["kmer_means"][v, s, :A] = w[at:at + 6 * A].copy().view(np.float64).reshape(A, 3)
                at += 6 * A
            assert at == int(voff[v0 + v + 1]), "genotype string: a record does not end where the next begins"
        out.append(d)
    return out


def diag_genotype_cluster(S, H, V, hap_allele, var_num_alleles, var_has_dependency, h1, h2, freq, stats, ploidy, min_gpp, min_kmers, min_fraction):
    """bt_diag_genotype_cluster: the device's summary code run on the host for one cluster given as bth_cluster_genotypes takes it -> the word string"""
    arrs = [np.ascontiguousarray(hap_allele, np.uint16).reshape(-1), np.ascontiguousarray(var_num_alleles, np.uint16), np.ascontiguousarray(var_has_dependency, np.uint8),
            np.ascontiguousarray(h1, np.uint16), np.ascontiguousarray(h2, np.uint16), np.ascontiguousarray(freq, np.uint32).reshape(-1),
            np.ascontiguousarray(stats, np.float64).reshape(-1), np.ascontiguousarray(ploidy, np.uint8)]
    nd = len(arrs[3])
    arrs = [a if a.size else np.zeros(1, a.dtype) for a in arrs]
    f, keep = _genotype_filters(min_gpp, min_kmers, min_fraction)
    n = C.c_uint64()
    args = [S, H, V, _np_ptr(arrs[0]), _np_ptr(arrs[1]), _np_ptr(arrs[2]), nd, _np_ptr(arrs[3]), _np_ptr(arrs[4]), _np_ptr(arrs[5]), _np_ptr(arrs[6]), _np_ptr(arrs[7]), C.addressof(f)]
    bt_diag_genotype_cluster(*args, None, 0, C.byref(n))   # (fails with "buffer too small" after setting the size)
    out = np.zeros(n.value, np.uint32)
    check(bt_diag_genotype_cluster(*args, _np_ptr(out), out.size, C.byref(n)))
    del keep
    return out


def diag_format_g6(values):
    """bt_diag_format_g6: the device's number formatter (printf's %g at precision 6) run on the host -> list of str, None where a value is not covered"""
    v = np.ascontiguousarray(values, np.float64).reshape(-1)
    text, lens = np.zeros(max(v.size, 1) * 16, np.uint8), np.zeros(max(v.size, 1), np.int32)
    check(bt_diag_format_g6(_np_ptr(v) if v.size else None, v.size, _np_ptr(text), _np_ptr(lens)))
    raw = text.tobytes()
    return [None if lens[i] < 0 else raw[16 * i:16 * i + int(lens[i])].decode() for i in range(v.size)]


def diag_genotype_text(words):
    """bt_diag_genotype_text: the device's text passes run on the host over a record string -> (text bytes, index words, number of not-covered variants)"""
    w = np.ascontiguousarray(words, np.uint32)
    nt, ni, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
    bt_diag_genotype_text(_np_ptr(w), w.size, None, 0, None, 0, C.byref(nt), C.byref(ni), C.byref(nc))   # (fails with "buffer too small" after setting the sizes)
    text, index = np.zeros(max(nt.value, 1), np.uint8), np.zeros(max(ni.value, 1), np.uint32)
    check(bt_diag_genotype_text(_np_ptr(w), w.size, _np_ptr(text), nt.value, _np_ptr(index), ni.value, C.byref(nt), C.byref(ni), C.byref(nc)))
    return text[:nt.value], index[:ni.value], nc.value


def genotype_text_sizes(ctx, d_words, num_words):
    """bt_genotype_text_sizes of a record string in device memory -> (text bytes, index words)"""
    nt, ni = C.c_uint64(), C.c_uint64()
    check(bt_genotype_text_sizes(ctx.h, d_words, num_words, C.byref(nt), C.byref(ni)))
    return nt.value, ni.value


def genotype_text(ctx, d_words, num_words):
    """bt_genotype_text over a record string in device memory (d_words: device pointer) -> (text bytes, index words, number of not-covered variants) on the host"""
    nt, ni = genotype_text_sizes(ctx, d_words, num_words)
    d_text, d_index = DeviceBuffer(ctx, nt), DeviceBuffer(ctx, ni * 4)
    try:
        t, i, nc = C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(bt_genotype_text(ctx.h, d_words, num_words, d_text.ptr, nt, d_index.ptr, ni, C.byref(t), C.byref(i), C.byref(nc)))
        return d_text.download(np.uint8, t.value), d_index.download(np.uint32, i.value), nc.value
    finally:
        d_text.free()
        d_index.free()


class DeflateStats(C.Structure):   # include/btgpu.h: bt_deflate_stats
    _fields_ = [(n, C.c_uint64) for n in ("pieces", "stored_pieces", "literals", "matches", "matched_bytes", "bytes_in", "bytes_out")] + [
        (n, C.c_double) for n in ("seconds_h2d", "seconds_kernels", "seconds_d2h", "seconds_host")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


bt_deflate_bound = _sig("bt_deflate_bound", [C.c_uint64, u64p])
bt_deflate = _sig("bt_deflate", [vp, vp, C.c_uint64, C.c_int, vp, C.c_uint64, u64p, C.POINTER(DeflateStats)])
bt_gzip_save = _sig("bt_gzip_save", [vp, C.c_char_p, vp, C.c_uint64, C.c_uint32, C.POINTER(DeflateStats)])
bt_diag_deflate = _sig("bt_diag_deflate", [vp, C.c_uint64, C.c_int, vp, C.c_uint64, u64p, C.POINTER(DeflateStats)])


def _bytes_array(data):
    return np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)


def deflate_bound(n):
    """bt_deflate_bound: the largest raw deflate stream bt_deflate / bt_diag_deflate produce for n bytes"""
    cap = C.c_uint64()
    check(bt_deflate_bound(n, C.byref(cap)))
    return cap.value


def diag_deflate(data, last=True):
    """bt_diag_deflate: the device's compressor run on the host (a team of one thread) -> (raw deflate stream as bytes, stats dictionary)"""
    a = _bytes_array(data)
    out, n, st = np.zeros(deflate_bound(a.size), np.uint8), C.c_uint64(), DeflateStats()
    check(bt_diag_deflate(_np_ptr(a) if a.size else None, a.size, int(bool(last)), _np_ptr(out), out.size, C.byref(n), C.byref(st)))
    return out[:n.value].tobytes(), st.as_dict()


def deflate(ctx, data, last=True):
    """bt_deflate over a host buffer: uploaded, compressed on the device, downloaded -> (raw deflate stream as bytes, stats dictionary)"""
    a = _bytes_array(data)
    cap = deflate_bound(a.size)
    d_in, d_out = DeviceBuffer(ctx, a.size), DeviceBuffer(ctx, cap)
    try:
        if a.size:
            d_in.upload(a)
        n, st = C.c_uint64(), DeflateStats()
        check(bt_deflate(ctx.h, d_in.ptr if a.size else None, a.size, int(bool(last)), d_out.ptr, cap, C.byref(n), C.byref(st)))
        return d_out.download(np.uint8, n.value).tobytes(), st.as_dict()
    finally:
        d_in.free()
        d_out.free()


def gzip_save(ctx, path, data, threads=1):
    """bt_gzip_save: data -> the file `path`, one gzip member compressed on the device -> stats dictionary"""
    a = _bytes_array(data)
    st = DeflateStats()
    check(bt_gzip_save(ctx.h, os.fsencode(path), _np_ptr(a) if a.size else None, a.size, threads, C.byref(st)))
    return st.as_dict()


bt_bgzf_bound = _sig("bt_bgzf_bound", [C.c_uint64, u64p, u64p])
bt_bgzf = _sig("bt_bgzf", [vp, vp, C.c_uint64, C.c_int, vp, C.c_uint64, u64p, vp, C.POINTER(DeflateStats)])
bt_bgzf_save = _sig("bt_bgzf_save", [vp, C.c_char_p, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.POINTER(DeflateStats)])
bt_diag_bgzf = _sig("bt_diag_bgzf", [vp, C.c_uint64, C.c_int, vp, C.c_uint64, u64p, vp, C.POINTER(DeflateStats)])
bt_diag_crc32 = _sig("bt_diag_crc32", [vp, C.c_uint64, C.POINTER(C.c_uint32)])


def bgzf_bound(n):
    """bt_bgzf_bound -> (the largest BGZF stream bt_bgzf / bt_diag_bgzf produce for n bytes, EOF block included; the number of data blocks)"""
    cap, blocks = C.c_uint64(), C.c_uint64()
    check(bt_bgzf_bound(n, C.byref(cap), C.byref(blocks)))
    return cap.value, blocks.value


def diag_bgzf(data, eof=True):
    """bt_diag_bgzf: the device's BGZF writer run on the host (a team of one thread) -> (stream as bytes, block offsets [blocks + 1] as a list, stats)"""
    a = _bytes_array(data)
    cap, blocks = bgzf_bound(a.size)
    out, offs, n, st = np.zeros(cap, np.uint8), np.zeros(blocks + 1, np.uint64), C.c_uint64(), DeflateStats()
    check(bt_diag_bgzf(_np_ptr(a) if a.size else None, a.size, int(bool(eof)), _np_ptr(out), out.size, C.byref(n), _np_ptr(offs), C.byref(st)))
    return out[:n.value].tobytes(), [int(o) for o in offs], st.as_dict()


def diag_crc32(data):
    """bt_diag_crc32: the blocks' CRC-32 routine run on the host -> zlib's crc32 of data"""
    a = _bytes_array(data)
    crc = C.c_uint32()
    check(bt_diag_crc32(_np_ptr(a) if a.size else None, a.size, C.byref(crc)))
    return crc.value


def bgzf(ctx, data, eof=True):
    """bt_bgzf over a host buffer: uploaded, written as BGZF on the device, downloaded -> (stream as bytes, block offsets as a list, stats)"""
    a = _bytes_array(data)
    cap, blocks = bgzf_bound(a.size)
    d_in, d_out = DeviceBuffer(ctx, a.size), DeviceBuffer(ctx, cap)
    try:
        if a.size:
            d_in.upload(a)
        offs, n, st = np.zeros(blocks + 1, np.uint64), C.c_uint64(), DeflateStats()
        check(bt_bgzf(ctx.h, d_in.ptr if a.size else None, a.size, int(bool(eof)), d_out.ptr, cap, C.byref(n), _np_ptr(offs), C.byref(st)))
        return d_out.download(np.uint8, n.value).tobytes(), [int(o) for o in offs], st.as_dict()
    finally:
        d_in.free()
        d_out.free()


def bgzf_save(ctx, path, data, threads=1):
    """bt_bgzf_save: data -> the file `path`, BGZF written on the device, EOF block included -> (block offsets in the file as a list, stats)"""
    a = _bytes_array(data)
    offs, st = np.zeros(bgzf_bound(a.size)[1] + 1, np.uint64), DeflateStats()
    check(bt_bgzf_save(ctx.h, os.fsencode(path), _np_ptr(a) if a.size else None, a.size, threads, _np_ptr(offs), offs.size, C.byref(st)))
    return [int(o) for o in offs], st.as_dict()


BGZF_BLOCK = np.dtype([("in_offset", np.uint64), ("out_offset", np.uint64), ("in_size", np.uint32), ("isize", np.uint32)])   # include/btgpu.h: bt_bgzf_block


class BamStats(C.Structure):   # include/btgpu.h: bt_bam_stats
    _fields_ = [("kept", C.c_uint64), ("skipped", C.c_uint64), ("bases", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


bt_bgzf_scan_blocks = _sig("bt_bgzf_scan_blocks", [vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, u64p])
bt_bgzf_inflate = _sig("bt_bgzf_inflate", [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64])
bt_diag_bgzf_inflate = _sig("bt_diag_bgzf_inflate", [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64])
bt_bam_reads_text = _sig("bt_bam_reads_text", [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p, C.POINTER(BamStats)])
bt_diag_bam_reads_text = _sig("bt_diag_bam_reads_text", [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p, C.POINTER(BamStats)])
bt_bam_scan_create = _sig("bt_bam_scan_create", [vp, C.c_uint64, C.c_uint32, C.POINTER(vp)])
bt_bam_scan_text = _sig("bt_bam_scan_text", [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(vp), u64p, C.POINTER(BamStats)])
bt_bam_scan_finish = _sig("bt_bam_scan_finish", [vp])
bt_bam_scan_destroy = _sig("bt_bam_scan_destroy", [vp], None)
BAM_SKIP_FLAGS = 0x900   # secondary and supplementary alignments: every read once


def bgzf_scan_blocks(data):
    """bt_bgzf_scan_blocks (no GPU): a buffer that starts at a BGZF block boundary -> (table of its whole blocks as a BGZF_BLOCK array, bytes they take,
    sum of their ISIZEs); a trailing partial block is not taken"""
    a = _bytes_array(data)
    n, used, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(bt_bgzf_scan_blocks(_np_ptr(a) if a.size else None, a.size, None, 0, C.byref(n), C.byref(used), C.byref(total)))
    blocks = np.zeros(n.value, BGZF_BLOCK)
    check(bt_bgzf_scan_blocks(_np_ptr(a) if a.size else None, a.size, _np_ptr(blocks), blocks.size, C.byref(n), C.byref(used), C.byref(total)))
    return blocks, used.value, total.value


def _bgzf_job(data, blocks, out_bytes):
    a = _bytes_array(data)
    if blocks is None:
        blocks, used, total = bgzf_scan_blocks(a)
        if used != a.size:
            raise BtError(f"BGZF block at offset {used}: incomplete (the buffer ends inside it)")
    blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK)
    if out_bytes is None:
        out_bytes = int(max((int(b["out_offset"]) + int(b["isize"]) for b in blocks), default=0))
    return a, blocks, out_bytes


def diag_bgzf_inflate(data, blocks=None, out=None, capacity=None, out_bytes=None, file_offset=0):
    """bt_diag_bgzf_inflate: the device's BGZF reader run on the host (a team of one thread) -> the blocks' data as bytes.  blocks: a table other than
    bgzf_scan_blocks(data)'s; out: a uint8 array to write into (capacity: how much of it the call may use)"""
    a, blocks, out_bytes = _bgzf_job(data, blocks, out_bytes)
    if out is None:
        out = np.zeros(max(out_bytes, 1), np.uint8)
    cap = out.size if capacity is None else capacity
    check(bt_diag_bgzf_inflate(_np_ptr(a) if a.size else None, a.size, _np_ptr(blocks) if blocks.size else None, blocks.size, _np_ptr(out), cap, out_bytes, file_offset))
    return out[:out_bytes].tobytes()


def bgzf_inflate(ctx, data, blocks=None, capacity=None, out_bytes=None, file_offset=0, guard=0, keep=None):
    """bt_bgzf_inflate over a host buffer: blocks and table uploaded, inflated on the device, downloaded -> the blocks' data as bytes.  guard: bytes
    allocated behind the output (preset to 0xA5) and returned with it; keep: a dict that receives the output as downloaded even when the call fails"""
    a, blocks, out_bytes = _bgzf_job(data, blocks, out_bytes)
    cap = out_bytes if capacity is None else capacity
    d_in, d_tab, d_out = DeviceBuffer(ctx, a.size), DeviceBuffer(ctx, blocks.nbytes), DeviceBuffer(ctx, max(cap, out_bytes) + guard)
    try:
        if a.size:
            d_in.upload(a)
        if blocks.size:
            d_tab.upload(blocks)
        check(bt_memset(ctx.h, d_out.ptr, 0xA5, d_out.nbytes))
        try:
            check(bt_bgzf_inflate(ctx.h, d_in.ptr if a.size else None, a.size, d_tab.ptr if blocks.size else None, blocks.size, d_out.ptr, cap, out_bytes, file_offset))
        finally:
            if keep is not None:
                ctx.sync()
                keep["out"] = d_out.download(np.uint8, out_bytes + guard).tobytes()
        return d_out.download(np.uint8, out_bytes + guard).tobytes()
    finally:
        d_in.free()
        d_tab.free()
        d_out.free()


def diag_bam_reads_text(bam, skip_flags=BAM_SKIP_FLAGS, capacity=None):
    """bt_diag_bam_reads_text (no GPU): inflated BAM records from a record boundary on -> (reads text as bytes, offset of the first record that is not
    whole, stats)"""
    a = _bytes_array(bam)
    cap = a.size if capacity is None else capacity
    out, n, used, st = np.full(cap + 16, 0xA5, np.uint8), C.c_uint64(), C.c_uint64(), BamStats()
    check(bt_diag_bam_reads_text(_np_ptr(a) if a.size else None, a.size, skip_flags, _np_ptr(out), cap, C.byref(n), C.byref(used), C.byref(st)))
    assert (out[cap:] == 0xA5).all()
    return out[:n.value].tobytes(), used.value, st.as_dict()


def bam_reads_text(ctx, bam, skip_flags=BAM_SKIP_FLAGS, capacity=None, misalign=0):
    """bt_bam_reads_text over a host buffer (uploaded `misalign` bytes into its allocation) -> (reads text as bytes, offset of the first record that is not
    whole, stats)"""
    a = _bytes_array(bam)
    cap = a.size if capacity is None else capacity
    d_in, d_out = DeviceBuffer(ctx, a.size + misalign), DeviceBuffer(ctx, cap + 16)
    try:
        if a.size:
            check(bt_memcpy_h2d(ctx.h, d_in.ptr + misalign, _np_ptr(a), a.size))
        check(bt_memset(ctx.h, d_out.ptr, 0xA5, d_out.nbytes))
        n, used, st = C.c_uint64(), C.c_uint64(), BamStats()
        check(bt_bam_reads_text(ctx.h, d_in.ptr + misalign if a.size else None, a.size, skip_flags, d_out.ptr, cap, C.byref(n), C.byref(used), C.byref(st)))
        out = d_out.download(np.uint8, cap + 16)
        assert (out[cap:] == 0xA5).all()
        return out[:n.value].tobytes(), used.value, st.as_dict()
    finally:
        d_in.free()
        d_out.free()


class _Scan:
    """What the stream-object wrappers share: a call's text downloaded, and the handle's end.  A subclass creates self.h and names its library's destroy function in
    _destroy."""

    def _download(self, d, n, st):
        out = np.empty(n, np.uint8)
        if n:
            check(bt_memcpy_d2h(self.ctx.h, _np_ptr(out), d, n))
        return out.tobytes(), st

    def text_bytes(self, *args, **kw):
        """text(), downloaded -> (bytes, stats)"""
        return self._download(*self.text(*args, **kw))

    def close(self):
        if self.h:
            self._destroy(self.h)
            self.h = None


class _FastqScan(_Scan):
    """The two FASTQ stream objects: the same calls over the functions the subclass names in _text and _finish."""

    def text(self, data):
        """-> (device pointer of the text, valid until the next call; its length; this call's stats)"""
        a = _bytes_array(data)
        d, n, st = vp(), C.c_uint64(), FastqStats()
        check(self._text(self.h, _np_ptr(a) if a.size else None, a.size, C.byref(d), C.byref(n), C.byref(st)))
        return d.value, n.value, st.as_dict()

    def finish(self):
        """the carried tail as the file's end -> (device pointer of its text, its length, stats)"""
        d, n, st = vp(), C.c_uint64(), FastqStats()
        check(self._finish(self.h, C.byref(d), C.byref(n), C.byref(st)))
        return d.value, n.value, st.as_dict()

    def finish_bytes(self):
        """finish(), downloaded -> (bytes, stats)"""
        return self._download(*self.finish())


class BamScan(_Scan):
    """bt_bam_scan: slabs of whole BGZF blocks of a BAM file -> reads text in device memory"""
    _destroy = bt_bam_scan_destroy

    def __init__(self, ctx, max_in_bytes, skip_flags=BAM_SKIP_FLAGS):
        self.ctx = ctx
        h = vp()
        check(bt_bam_scan_create(ctx.h, max_in_bytes, skip_flags, C.byref(h)))
        self.h = h.value

    def text(self, blocks, skip_first_bytes=0):
        """-> (device pointer of the text, valid until the next call; its length; this call's stats)"""
        a = _bytes_array(blocks)
        d, n, st = vp(), C.c_uint64(), BamStats()
        check(bt_bam_scan_text(self.h, _np_ptr(a) if a.size else None, a.size, skip_first_bytes, C.byref(d), C.byref(n), C.byref(st)))
        return d.value, n.value, st.as_dict()

    def finish(self):
        check(bt_bam_scan_finish(self.h))


class FastqStats(C.Structure):   # include/btgpu.h: bt_fastq_stats
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("lines", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


bt_fastq_reads_text = _sig("bt_fastq_reads_text", [vp, vp, C.c_uint64, C.c_int, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(FastqStats)])
bt_diag_fastq_reads_text = _sig("bt_diag_fastq_reads_text", [vp, C.c_uint64, C.c_int, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(FastqStats)])
bt_fastq_count_tile = _sig("bt_fastq_count_tile", [], C.c_uint32)
bt_fastq_scan_create = _sig("bt_fastq_scan_create", [vp, C.c_uint64, C.POINTER(vp)])
bt_fastq_scan_text = _sig("bt_fastq_scan_text", [vp, vp, C.c_uint64, C.POINTER(vp), u64p, C.POINTER(FastqStats)])
bt_fastq_scan_finish = _sig("bt_fastq_scan_finish", [vp, C.POINTER(vp), u64p, C.POINTER(FastqStats)])
bt_fastq_scan_destroy = _sig("bt_fastq_scan_destroy", [vp], None)
FASTQ_COUNT_TILE = int(bt_fastq_count_tile())   # bytes per workgroup of the kernels that find the lines, counted from the data's first byte


def diag_fastq_reads_text(fastq, final=True, first_line=1, capacity=None, null=None):
    """bt_diag_fastq_reads_text (no GPU): FASTQ text from a record boundary on -> (reads text as bytes, offset of the first record that is not whole,
    stats).  null: "text" / "text_bytes" / "consumed" passes that argument as NULL"""
    a = _bytes_array(fastq)
    cap = a.size if capacity is None else capacity
    out, n, used, st = np.full(cap + 16, 0xA5, np.uint8), C.c_uint64(), C.c_uint64(), FastqStats()
    try:
        check(bt_diag_fastq_reads_text(_np_ptr(a) if a.size else None, a.size, int(bool(final)), first_line, None if null == "text" else _np_ptr(out), cap,
                                       None if null == "text_bytes" else C.byref(n), None if null == "consumed" else C.byref(used), C.byref(st)))
    finally:
        assert (out[cap:] == 0xA5).all()
    assert (out[n.value:cap] == 0xA5).all()
    return out[:n.value].tobytes(), used.value, st.as_dict()


def fastq_reads_text(ctx, fastq, final=True, first_line=1, capacity=None, misalign=0):
    """bt_fastq_reads_text over a host buffer (uploaded `misalign` bytes into its allocation) -> (reads text as bytes, offset of the first record that is
    not whole, stats).  The bytes behind the text and behind the capacity are checked to be untouched."""
    a = _bytes_array(fastq)
    cap = a.size if capacity is None else capacity
    d_in, d_out = DeviceBuffer(ctx, a.size + misalign), DeviceBuffer(ctx, cap + 16)
    try:
        if a.size:
            check(bt_memcpy_h2d(ctx.h, d_in.ptr + misalign, _np_ptr(a), a.size))
        check(bt_memset(ctx.h, d_out.ptr, 0xA5, d_out.nbytes))
        n, used, st = C.c_uint64(), C.c_uint64(), FastqStats()
        try:
            check(bt_fastq_reads_text(ctx.h, d_in.ptr + misalign if a.size else None, a.size, int(bool(final)), first_line, d_out.ptr, cap, C.byref(n), C.byref(used), C.byref(st)))
        finally:
            ctx.sync()
            out = d_out.download(np.uint8, cap + 16)
            assert (out[cap:] == 0xA5).all()
        assert (out[n.value:cap] == 0xA5).all()
        return out[:n.value].tobytes(), used.value, st.as_dict()
    finally:
        d_in.free()
        d_out.free()


class FastqScan(_FastqScan):
    """bt_fastq_scan: slabs of whole BGZF blocks of a BGZF-compressed FASTQ file -> reads text in device memory"""
    _text, _finish, _destroy = bt_fastq_scan_text, bt_fastq_scan_finish, bt_fastq_scan_destroy

    def __init__(self, ctx, max_in_bytes):
        self.ctx = ctx
        h = vp()
        check(bt_fastq_scan_create(ctx.h, max_in_bytes, C.byref(h)))
        self.h = h.value


class GunzipStats(C.Structure):   # include/btgpu.h: bt_gunzip_stats
    _fields_ = [("rounds", C.c_uint64), ("candidates", C.c_uint64), ("links_verified", C.c_uint64), ("links_broken", C.c_uint64), ("blocks", C.c_uint64),
                ("out_bytes", C.c_uint64)]


def parse_gunzip_stats(st):
    """bt_gunzip_stats -> dict"""
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


_raw_args = [vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(GunzipStats)]
bt_inflate_raw = _sig("bt_inflate_raw", [vp] + _raw_args)
bt_diag_inflate_raw = _sig("bt_diag_inflate_raw", _raw_args)
bt_diag_gunzip_plausible = _sig("bt_diag_gunzip_plausible", [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp])
bt_gunzip_default_chunk_bytes = _sig("bt_gunzip_default_chunk_bytes", [], C.c_uint32)
bt_gunzip_expansion_budget = _sig("bt_gunzip_expansion_budget", [], C.c_uint32)
bt_fastq_gz_scan_create = _sig("bt_fastq_gz_scan_create", [vp, C.c_uint64, C.c_uint32, C.POINTER(vp)])
bt_fastq_gz_scan_text = _sig("bt_fastq_gz_scan_text", [vp, vp, C.c_uint64, C.POINTER(vp), u64p, C.POINTER(FastqStats)])
bt_fastq_gz_scan_finish = _sig("bt_fastq_gz_scan_finish", [vp, C.POINTER(vp), u64p, C.POINTER(FastqStats)])
bt_fastq_gz_scan_stats = _sig("bt_fastq_gz_scan_stats", [vp, C.POINTER(GunzipStats)])
bt_fastq_gz_scan_destroy = _sig("bt_fastq_gz_scan_destroy", [vp], None)
bt_diag_gunzip_stage_seconds = _sig("bt_diag_gunzip_stage_seconds", [C.POINTER(C.c_double), C.c_int], None)
GUNZIP_DEFAULT_CHUNK = int(bt_gunzip_default_chunk_bytes())
GUNZIP_EXPAND = int(bt_gunzip_expansion_budget())
GUNZIP_GUARD = 64   # bytes behind the capacity, preset to 0xA5 and checked


def _raw_result(out, cap, n, end, fin, crc, st):
    assert (out[cap:] == 0xA5).all(), "bytes written at or past the capacity"
    assert (out[n.value:cap] == 0xA5).all(), "bytes written past out_bytes"
    return {"data": out[:n.value].tobytes(), "end_bit": int(end.value), "stream_end": int(fin.value), "crc32": int(crc.value), "stats": parse_gunzip_stats(st)}


def diag_inflate_raw(data, start_bit=0, window=b"", chunk_bytes=0, capacity=None):
    """bt_diag_inflate_raw (no GPU): a raw deflate stream from the block boundary start_bit on, `window` = the output before it -> dict(data, end_bit,
    stream_end, crc32, stats).  capacity None: 16 MiB.  The bytes behind the output and behind the capacity are checked to be untouched."""
    a, w = _bytes_array(data), _bytes_array(window)
    cap = (16 << 20) if capacity is None else capacity
    out = np.full(cap + GUNZIP_GUARD, 0xA5, np.uint8)
    n, end, fin, crc, st = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32(), GunzipStats()
    check(bt_diag_inflate_raw(_np_ptr(a) if a.size else None, a.size, start_bit, _np_ptr(w) if w.size else None, w.size, chunk_bytes, _np_ptr(out), cap, C.byref(n), C.byref(end),
                              C.byref(fin), C.byref(crc), C.byref(st)))
    return _raw_result(out, cap, n, end, fin, crc, st)


def inflate_raw(ctx, data, start_bit=0, window=b"", chunk_bytes=0, capacity=None):
    """bt_inflate_raw over host buffers (uploaded) -> as diag_inflate_raw"""
    a, w = _bytes_array(data), _bytes_array(window)
    cap = (16 << 20) if capacity is None else capacity
    d_in, d_win, d_out = DeviceBuffer(ctx, a.size + 8), DeviceBuffer(ctx, w.size + 8), DeviceBuffer(ctx, cap + GUNZIP_GUARD)
    try:
        if a.size:
            d_in.upload(a)
        if w.size:
            d_win.upload(w)
        check(bt_memset(ctx.h, d_out.ptr, 0xA5, d_out.nbytes))
        n, end, fin, crc, st = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32(), GunzipStats()
        try:
            check(bt_inflate_raw(ctx.h, d_in.ptr if a.size else None, a.size, start_bit, d_win.ptr if w.size else None, w.size, chunk_bytes, d_out.ptr, cap, C.byref(n), C.byref(end),
                                 C.byref(fin), C.byref(crc), C.byref(st)))
        finally:
            ctx.sync()
            out = d_out.download(np.uint8, cap + GUNZIP_GUARD)
            assert (out[cap:] == 0xA5).all(), "bytes written at or past the capacity"
        return _raw_result(out, cap, n, end, fin, crc, st)
    finally:
        d_in.free()
        d_win.free()
        d_out.free()


def diag_gunzip_plausible(data, first_bit=0, n_bits=None):
    """bt_diag_gunzip_plausible (no GPU): the find stage's test at the bit offsets first_bit .. first_bit + n_bits (default: to the data's end) -> uint8 array
    of 0 / 1"""
    a = _bytes_array(data)
    if n_bits is None:
        n_bits = 8 * a.size - first_bit
    flags = np.full(max(n_bits, 0) + 16, 0xA5, np.uint8)
    check(bt_diag_gunzip_plausible(_np_ptr(a) if a.size else None, a.size, first_bit, n_bits, _np_ptr(flags)))
    assert (flags[n_bits:] == 0xA5).all()
    return flags[:n_bits].copy()


def gunzip_stage_seconds(reset=False):
    """bt_diag_gunzip_stage_seconds -> dict of wall seconds per stage (find, decode, windows, resolve, crc)"""
    out = (C.c_double * 5)()
    bt_diag_gunzip_stage_seconds(out, int(bool(reset)))
    return dict(zip(("find", "decode", "windows", "resolve", "crc"), (float(x) for x in out)))


class FastqGzScan(_FastqScan):
    """bt_fastq_gz_scan: any cuts of an ordinary gzip FASTQ file (one or more long members) -> reads text in device memory.  The file has to end at a member
    boundary: finish() says so when it does not."""
    _text, _finish, _destroy = bt_fastq_gz_scan_text, bt_fastq_gz_scan_finish, bt_fastq_gz_scan_destroy

    def __init__(self, ctx, max_in_bytes, chunk_bytes=0):
        self.ctx = ctx
        h = vp()
        check(bt_fastq_gz_scan_create(ctx.h, max_in_bytes, chunk_bytes, C.byref(h)))
        self.h = h.value

    def stats(self):
        """the sums of the inflate calls' stats so far"""
        st = GunzipStats()
        check(bt_fastq_gz_scan_stats(self.h, C.byref(st)))
        return parse_gunzip_stats(st)


def parse_genotype_text(text, index):
    """text and index of bt_gibbs_genotype_text / bt_genotype_text / bt_diag_genotype_text (layout: include/btgpu.h) -> per variant, in the string's order, a
    dictionary with the three pieces as str — "stats", "cover", "samples" with every GQ (derived here from the cell's best posterior, as the host layer
    does) spliced into its slot — and "A", "total_count", "max_alt_acp" (float32), "flags" (1 = not covered)"""
    index = np.ascontiguousarray(index, np.uint32)
    raw = np.ascontiguousarray(text, np.uint8).tobytes()
    Cn, NV, S = int(index[0]), int(index[1]), int(index[2])
    var = index[5 + Cn:5 + Cn + 9 * NV].reshape(NV, 9)
    cells = index[5 + Cn + 9 * NV:5 + Cn + 9 * NV + 2 * NV * S].reshape(NV, S, 2)
    out = []
    for v in range(NV):
        off = int(var[v, 0]) | (int(var[v, 1]) << 32)
        n_stats, n_cover, n_samples = (int(x) for x in var[v, 2:5])
        samples = raw[off + n_stats + n_cover:off + n_stats + n_cover + n_samples]
        parts, at = [], 0
        for s in range(S):
            slot = int(cells[v, s, 1])
            if slot == 0xFFFFFFFF:
                continue
            parts.append(samples[at:slot] + str(genotype_quality(cells[v, s, 0:1].view(np.float32)[0])).encode())
            at = slot
        parts.append(samples[at:])
        out.append({"stats": raw[off:off + n_stats].decode(), "cover": raw[off + n_stats:off + n_stats + n_cover].decode(), "samples": b"".join(parts).decode(),
                    "A": int(var[v, 5]), "total_count": int(var[v, 6]), "max_alt_acp": var[v, 7:8].view(np.float32)[0], "flags": int(var[v, 8])})
    return out


class Gibbs:
    """A batch of variant-cluster groups on one GPU (bt_gibbs_*).  `flat` is a dict as produced by bayestyper_amd.synth."""

    def __init__(self, ctx, flat, lut_g, lut_n, **kw):
        from . import synth

        self.ctx, self.flat = ctx, flat
        self.S, self.C, self.G = flat["S"], flat["num_clusters"], flat["num_groups"]
        self.params, self.batch, self._keep = synth.to_ctypes(flat, **kw)
        h = vp()
        check(bt_gibbs_create(ctx.h, C.addressof(self.params), C.addressof(self.batch), C.byref(h)))
        self.h = h.value
        if lut_g is not None:
            self.set_lut(lut_g, lut_n)

    @classmethod
    def _from_handle(cls, ctx, h, flat, params, keep):
        """a sampler the library built from a source (GibbsSource.sampler); `flat` holds S, num_groups, num_clusters, group_cluster_off of ITS groups"""
        g = cls.__new__(cls)
        g.ctx, g.flat, g.h = ctx, flat, h
        g.S, g.C, g.G = flat["S"], flat["num_clusters"], flat["num_groups"]
        g.params, g.batch, g._keep = params, None, keep
        return g

    def set_lut(self, lut_g, lut_n):
        lut_g, lut_n = np.ascontiguousarray(lut_g, np.float64), np.ascontiguousarray(lut_n, np.float64)
        check(bt_gibbs_set_lut(self.h, _np_ptr(lut_g), _np_ptr(lut_n)))

    def set_noise_lut(self, lut_n):
        lut_n = np.ascontiguousarray(lut_n, np.float64)
        check(bt_gibbs_set_noise_lut(self.h, _np_ptr(lut_n)))

    def run(self):
        check(bt_gibbs_run(self.h))

    def init_chain(self, c):
        check(bt_gibbs_init_chain(self.h, c))

    def sweep(self, n, collect):
        check(bt_gibbs_sweep(self.h, n, int(collect)))

    def noise_counts(self, zero_first=True):
        d = self.ctx.buffer(self.S * 256 * 8)
        check(bt_gibbs_noise_counts(self.h, d.ptr, int(zero_first)))
        self.ctx.sync()
        out = d.download(np.uint64, self.S * 256)
        d.free()
        return out

    def noise_iteration(self, lut_n, collect):
        """bt_gibbs_noise_iteration: (the table for this iteration's sweep or None;) one sweep; noise counts [S*256] + clearGenotyperCache"""
        if lut_n is not None:
            lut_n = np.ascontiguousarray(lut_n, np.float64)
        h = np.zeros(self.S * 256, np.uint64)
        check(bt_gibbs_noise_iteration(self.h, _np_ptr(lut_n) if lut_n is not None else None, int(collect), _np_ptr(h)))
        return h

    def noise_chain_begin(self, num_iterations, first_collect):
        """bt_gibbs_noise_chain_begin -> True when the chain runs as one resident launch (then noise_chain_step per iteration, noise_chain_end)"""
        r = C.c_int(0)
        check(bt_gibbs_noise_chain_begin(self.h, num_iterations, first_collect, C.byref(r)))
        return bool(r.value)

    def noise_chain_step(self, lut_n):
        if lut_n is not None:
            lut_n = np.ascontiguousarray(lut_n, np.float64)
        h = np.zeros(self.S * 256, np.uint64)
        check(bt_gibbs_noise_chain_step(self.h, _np_ptr(lut_n) if lut_n is not None else None, _np_ptr(h)))
        return h

    def noise_chain_end(self):
        check(bt_gibbs_noise_chain_end(self.h))

    def reset_groups(self):
        check(bt_gibbs_reset_groups(self.h))

    def posterior_summary(self):
        """bt_gibbs_posterior_summary -> uint32 [C, S, 2] on the host (the device buffer is what a multi-GPU run gathers)"""
        buf = DeviceBuffer(self.ctx, self.C * self.S * 2 * 4)
        check(bt_gibbs_posterior_summary(self.h, buf.ptr))
        self.ctx.sync()
        out = buf.download(np.uint32, self.C * self.S * 2).reshape(self.C, self.S, 2)
        buf.free()
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(bt_gibbs_device_bytes(self.h, C.byref(b)))
        return b.value

    def timeline_enable(self, n):
        """bt_gibbs_timeline_enable: room for the wavefront records of n sampling launches (0: off)"""
        check(bt_gibbs_timeline_enable(self.h, n))

    def timeline_sizes(self):
        """-> (records, launches, dropped, tick_khz)"""
        r, l, d, k = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(bt_gibbs_timeline_sizes(self.h, C.byref(r), C.byref(l), C.byref(d), C.byref(k)))
        return r.value, l.value, d.value, k.value

    def timeline(self):
        """bt_gibbs_timeline_fetch -> (TIMELINE_RECORD array, tick_khz, dropped)"""
        n, _, dropped, khz = self.timeline_sizes()
        rec = np.zeros(n, TIMELINE_RECORD)
        got = C.c_uint64()
        check(bt_gibbs_timeline_fetch(self.h, _np_ptr(rec) if n else None, n, C.byref(got)))
        return rec[: got.value], khz, dropped

    def trace_enable(self, n):
        check(bt_gibbs_trace_enable(self.h, n))
        self._trace_n = n

    def trace(self):
        """-> list per group of arrays [sweeps][vertex][S]"""
        goff = self.flat["group_cluster_off"]
        nv = (goff[1:] - goff[:-1]).astype(np.int64)
        total = int((nv * self._trace_n * self.S).sum())
        buf = np.zeros(max(total, 1), np.uint32)
        n0 = C.c_uint64()
        check(bt_gibbs_trace_fetch(self.h, _np_ptr(buf), len(buf), C.byref(n0)))
        out, off = [], 0
        for g in range(self.G):
            w = int(nv[g]) * self._trace_n * self.S
            out.append(buf[off:off + w].reshape(self._trace_n, int(nv[g]), self.S))
            off += w
        return out

    def results(self):
        self.ctx.sync()
        nd, nc = C.c_uint64(), C.c_uint64()
        check(bt_gibbs_result_sizes(self.h, C.byref(nd), C.byref(nc)))
        nd, nc = nd.value, nc.value
        dip_off = np.zeros(self.C + 1, np.uint64)
        cell_off = np.zeros(self.C + 1, np.uint64)
        h1, h2 = np.zeros(max(nd, 1), np.uint16), np.zeros(max(nd, 1), np.uint16)
        freq = np.zeros(max(nd, 1) * self.S, np.uint32)
        stats = np.zeros(max(nc, 1) * 12, np.float64)
        check(bt_gibbs_result_fetch(self.h, _np_ptr(dip_off), _np_ptr(h1), _np_ptr(h2), _np_ptr(freq), _np_ptr(cell_off), _np_ptr(stats)))
        return {"dip_off": dip_off, "h1": h1[:nd], "h2": h2[:nd], "freq": freq[: nd * self.S].reshape(nd, self.S), "cell_off": cell_off,
                "stats": stats[: nc * 12].reshape(nc, 3, 4)}

    def result_words(self):
        """the results as one word string in DEVICE memory (bt_gibbs_result_words): (device pointer, words); the sampler owns the buffer"""
        p, n = vp(), C.c_uint64()
        check(bt_gibbs_result_words(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def sparse_forms(self):
        """bt_gibbs_sparse_forms -> uint32 [C]: 0 dense, 1 sparse on lists, 2 sparse on packed words, 0xFFFFFFFF not constructed"""
        out = np.zeros(self.C, np.uint32)
        check(bt_gibbs_sparse_forms(self.h, _np_ptr(out)))
        return out

    def result_words_host(self):
        p, n = self.result_words()
        out = np.zeros(n, np.uint32)
        check(bt_memcpy_d2h(self.ctx.h, _np_ptr(out), p, out.nbytes))
        return out

    def genotypes(self, min_gpp, min_kmers, min_fraction):
        """bt_gibbs_genotypes: the launch's genotype summaries computed on the device -> the word string on the host (parse_genotype_words)"""
        f, keep = _genotype_filters(min_gpp, min_kmers, min_fraction)
        if len(keep) != self.S:
            raise ValueError("one min_fraction_observed_kmers per sample")
        p, n = vp(), C.c_uint64()
        check(bt_gibbs_genotypes(self.h, C.addressof(f), C.byref(p), C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        check(bt_memcpy_d2h(self.ctx.h, _np_ptr(out), p, out.nbytes))
        return out

    def genotype_text(self, min_gpp, min_kmers, min_fraction):
        """bt_gibbs_genotype_text: the launch's genotype text formatted on the device -> (text bytes, index words, number of not-covered variants) on
        the host (parse_genotype_text)"""
        f, keep = _genotype_filters(min_gpp, min_kmers, min_fraction)
        if len(keep) != self.S:
            raise ValueError("one min_fraction_observed_kmers per sample")
        pt, pi, nt, ni, nc = vp(), vp(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(bt_gibbs_genotype_text(self.h, C.addressof(f), C.byref(pt), C.byref(nt), C.byref(pi), C.byref(ni), C.byref(nc)))
        text, index = np.zeros(nt.value, np.uint8), np.zeros(ni.value, np.uint32)
        if text.size:
            check(bt_memcpy_d2h(self.ctx.h, _np_ptr(text), pt, text.nbytes))
        check(bt_memcpy_d2h(self.ctx.h, _np_ptr(index), pi, index.nbytes))
        return text, index, nc.value

    def close(self):
        if self.h:
            bt_gibbs_destroy(self.h)
            self.h = None


SOURCE_FIELDS = [("group_ploidy", np.uint8), ("group_sources", np.uint32), ("edges", np.uint32), ("hap_kmer_mult", np.uint8), ("kmer_has_counts", np.uint8),
                 ("kmer_counts", np.uint8), ("kmer_ic_mult", np.uint8), ("kmer_shared", np.int32), ("kv_off", np.uint32), ("kv_var", np.uint16), ("kv_bits", np.uint32),
                 ("unique_idx", np.uint32), ("multi_idx", np.uint32), ("hap_allele", np.uint16), ("hapnest_off", np.uint32), ("hapnest_idx", np.uint32),
                 ("var_num_alleles", np.uint16), ("var_has_dependency", np.uint8), ("nestdep_cluster", np.uint32), ("nestdep_var_off", np.uint32), ("nestdep_var", np.uint16),
                 ("group_num_shared", np.uint32), ("kmer_off", np.uint32), ("unique_off", np.uint32), ("multi_off", np.uint32)]   # include/btgpu.h: bt_gibbs_source_arrays


class _SourceArrays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _ in SOURCE_FIELDS]


class GibbsSource:
    """A unit's flat batch arrays resident on the device (bt_gibbs_source_*), and samplers over any selection of its groups.
    `flat`: the batch's dict (synth.flatten layout); from_paths needs only its per-group / per-cluster / haplotype / variant / nested-dependency fields."""

    def __init__(self, ctx, h, flat):
        self.ctx, self.h, self.flat = ctx, h, flat
        self.S, self.G = flat["S"], flat["num_groups"]

    @classmethod
    def from_batch(cls, ctx, flat):
        from . import synth

        _, batch, keep = synth.to_ctypes(flat)
        h = vp()
        check(bt_gibbs_source_create(ctx.h, flat["S"], C.addressof(batch), C.byref(h)))
        del keep
        return cls(ctx, h.value, flat)

    @classmethod
    def from_paths(cls, ctx, paths, structure):
        """bt_gibbs_source_create_from_paths: takes the device candidates out of `paths` (Paths.candidates_device); `structure`: synth_graphs.gibbs_structure's dict"""
        from . import synth

        batch, keep = synth.GibbsBatch(), []
        batch.num_groups, batch.num_clusters = structure["num_groups"], structure["num_clusters"]
        for n in synth._BATCH_PTRS:
            a = structure.get(n)
            if a is None:
                continue   # NULL: comes from the paths handle
            a = np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))
            keep.append(a)
            setattr(batch, n, a.ctypes.data)
        h = vp()
        check(bt_gibbs_source_create_from_paths(ctx.h, structure["S"], paths.h, C.addressof(batch), C.byref(h)))
        return cls(ctx, h.value, structure)

    def fetch(self):
        """bt_gibbs_source_fetch -> dict of the source's arrays (bt_gibbs_batch's names)"""
        counts = np.zeros(25, np.uint64)
        check(bt_gibbs_source_fetch(self.h, _np_ptr(counts), None))
        arrs = {name: np.zeros(max(int(counts[i]), 1), dt) for i, (name, dt) in enumerate(SOURCE_FIELDS)}
        out = _SourceArrays()
        for name, _ in SOURCE_FIELDS:
            setattr(out, name, arrs[name].ctypes.data)
        check(bt_gibbs_source_fetch(self.h, _np_ptr(counts), C.byref(out)))
        return {name: arrs[name][: int(counts[i])] for i, (name, _) in enumerate(SOURCE_FIELDS)}

    def device_bytes(self):
        b = C.c_uint64()
        check(bt_gibbs_source_device_bytes(self.h, C.byref(b)))
        return b.value

    def _params(self, **kw):
        from . import synth

        p, _, keep = synth.to_ctypes({"S": self.S, "gender": self.flat["gender"], "num_groups": 0, "num_clusters": 0, **{n: np.zeros(1, np.uint8) for n in synth._BATCH_PTRS}}, **kw)
        return p, keep

    def state_bytes(self, ids=None, **kw):
        p, keep = self._params(**kw)
        ids_a = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        b = C.c_uint64()
        check(bt_gibbs_state_bytes_from_source(self.h, C.addressof(p), None if ids_a is None else _np_ptr(ids_a), 0 if ids_a is None else len(ids_a), C.byref(b)))
        return b.value

    def sampler(self, params, ids=None, lut_g=None, lut_n=None):
        """bt_gibbs_create_from_source over the groups at positions `ids` of the source (None: all); params: keyword arguments of synth.to_ctypes"""
        p, keep = self._params(**params)
        goff = np.asarray(self.flat["group_cluster_off"], np.int64)
        sel = np.arange(self.G) if ids is None else np.asarray(ids, np.int64)
        nv = goff[sel + 1] - goff[sel]
        flat = {"S": self.S, "num_groups": len(sel), "num_clusters": int(nv.sum()), "group_cluster_off": np.concatenate([[0], np.cumsum(nv)]).astype(np.uint32)}
        ids_a = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        h = vp()
        check(bt_gibbs_create_from_source(self.h, self.ctx.h, C.addressof(p), None if ids_a is None else _np_ptr(ids_a), 0 if ids_a is None else len(ids_a), C.byref(h)))
        g = Gibbs._from_handle(self.ctx, h.value, flat, p, keep)
        if lut_g is not None:
            g.set_lut(lut_g, lut_n)
        return g

    def close(self):
        if self.h:
            bt_gibbs_source_destroy(self.h)
            self.h = None
