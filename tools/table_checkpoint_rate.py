"""Rates of the k-mer table checkpoint's kernels (profiles/table_checkpoint.txt): python tools/table_checkpoint_rate.py, from the repository root on the GPU box.
A 2^28-slot table holding 96.6 M random keys (the C3 shape), S = 3 and S = 10: the sizing call of bt_table_pack (the counting sweep alone), the whole call,
bt_table_unpack into a fresh table of the same size, and bt_table_save / bt_table_load through a file in the temporary directory."""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayestyper_amd import lib

K, N, PEAK = 55, 96_600_000, 8e12
ctx = lib.Ctx(0)
print(ctx.info(), flush=True)
for S in (3, 10):
    t = lib.Table(ctx, 1 << 27, S, K)
    rng = np.random.default_rng(S)
    for i in range(0, N, 1 << 24):
        m = min(1 << 24, N - i)
        keys = np.empty((m, 2), np.uint64)
        keys[:, 0] = rng.integers(0, 1 << 63, m, dtype=np.uint64)
        keys[:, 1] = rng.integers(0, 1 << 46, m, dtype=np.uint64)
        t.insert(keys, mark_parameter=True)
    st = t.status()
    rb, slot_bytes = t.record_bytes(), 4 * ((6 + ((S + 3) & ~3) // 4 + 3) & ~3)
    print(f"S={S}: {st}, record {rb} B, slot {slot_bytes} B", flush=True)
    n = C.c_uint64()
    timer = lib.Timer(ctx)
    buf = ctx.buffer(st["num_keys"] * rb)
    for rep in range(3):
        timer.start(); lib.check(lib.bt_table_pack(t.h, None, 0, C.byref(n))); timer.stop(); ctx.sync()
        count_ms = timer.elapsed_ms()
        timer.start(); lib.check(lib.bt_table_pack(t.h, buf.ptr, st["num_keys"], C.byref(n))); timer.stop(); ctx.sync()
        both_ms = timer.elapsed_ms()
        pack_ms = both_ms - count_ms
        rd, wr = st["capacity"] * slot_bytes, n.value * rb
        print(f"  rep {rep}: sizing pass {count_ms:.2f} ms = {rd / count_ms / 1e9 * 1e3:.0f} GB/s read ({rd / (count_ms * 1e-3) / PEAK:.1%} of 8 TB/s); "
              f"pack pass {pack_ms:.2f} ms: read {rd / 1e9:.2f} GB + written {wr / 1e9:.2f} GB = {(rd + wr) / pack_ms / 1e9 * 1e3:.0f} GB/s ({(rd + wr) / (pack_ms * 1e-3) / PEAK:.1%})", flush=True)
    for rep in range(2):
        d = lib.Table(ctx, 1 << 27, S, K)
        ctx.sync()
        timer.start(); d.unpack(buf, n.value); timer.stop(); ctx.sync()
        ms = timer.elapsed_ms()
        rd = n.value * rb
        print(f"  unpack rep {rep}: {ms:.2f} ms for {n.value} records = {n.value / ms / 1e6 * 1e3:.0f} M records/s; records read {rd / 1e9:.2f} GB, slots written {n.value * slot_bytes / 1e9:.2f} GB "
              f"(at least one 64-byte sector read and written per record: {(rd + 2 * 64 * n.value) / (ms * 1e-3) / PEAK:.1%} of 8 TB/s)", flush=True)
        assert d.status()["num_keys"] == n.value
        d.close()
    # save / load of the same table through a file
    path = os.path.join(tempfile.gettempdir(), f"table_checkpoint_rate_S{S}.ckpt")
    t0 = time.time(); t.save(path, "k=55\n"); t1 = time.time()
    size = os.path.getsize(path)
    h = C.c_void_p()
    t2 = time.time(); lib.check(lib.bt_table_load(ctx.h, path.encode(), b"k=55\n", C.byref(h))); t3 = time.time()
    lib.bt_table_destroy(h)
    os.remove(path)
    print(f"  save {t1 - t0:.2f} s, load {t3 - t2:.2f} s, file {size / 1e9:.2f} GB ({size / (t1 - t0) / 1e9:.2f} / {size / (t3 - t2) / 1e9:.2f} GB/s, page cache)", flush=True)
    buf.free()
    t.close()
ctx.close()
