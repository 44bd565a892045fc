"""Rate of the getKmerStats histogram kernel (bt_kmc_scan_kmer_stats) on device-resident records.  usage: kmer_stats_rate.py [records 2^30]
Two batches of k = 55 records (p = 3, 1-byte counters, 14-byte records), each a block of 2^20 host-made records replicated on the device:
  uniform: random k-mers, counts 1..255 (records spread over ~10^5 bins)
  one-bin: distinct k-mers that all hold 13 A, C, G and T after an AAA prefix, count 1 (every record in one bin)
Each batch: one warm-up pass, then REPS passes timed with events; the histogram is checked after every batch."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bayestyper_amd import lib  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 30
K, P, SUF, REC, BLOCK, REPS = 55, 3, 13, 14, 1 << 20, 3
assert R % BLOCK == 0


def pack(sym, counts):
    """(n, 52) symbol codes (A=0 C=1 G=2 T=3) + counts -> KMC records: 4 symbols per byte, first symbol in the top bits, then the counter"""
    s = sym.reshape(len(sym), SUF, 4).astype(np.uint8)
    suf = (s[:, :, 0] << 6) | (s[:, :, 1] << 4) | (s[:, :, 2] << 2) | s[:, :, 3]
    return np.ascontiguousarray(np.column_stack([suf, counts.astype(np.uint8)]))


rng = np.random.default_rng(1)
batches = {
    "uniform": pack(rng.integers(0, 4, size=(BLOCK, K - P)), rng.integers(1, 256, size=BLOCK)),
    "one-bin": pack(rng.permuted(np.tile(np.repeat(np.arange(4), 13), (BLOCK, 1)), axis=1), np.ones(BLOCK, np.int64)),
}
ctx = lib.Ctx(0)
lut = np.full(4 ** P + 1, R, np.uint64)
lut[0] = 0                                  # every record has the prefix AAA
bins = lib.kmer_stats_bins(K)
ncomp = bins // 256
hist = ctx.buffer(8 * bins)
over = ctx.buffer(8)
timer = lib.Timer(ctx)
print(f"# kmer_stats_rate: {R} records per pass ({R * REC / 1e9:.1f} GB), {REPS} timed passes per batch, k={K} p={P} record {REC} B; {time.strftime('%Y-%m-%d %H:%M:%S')}")
for name, block in batches.items():
    assert block.shape == (BLOCK, REC)
    d = ctx.buffer(R * REC)
    blk = ctx.to_device(block)
    for i in range(R // BLOCK):
        lib.check(lib.bt_memcpy_d2d(ctx.h, d.ptr + i * BLOCK * REC, blk.ptr, BLOCK * REC))
    blk.free()
    sc = lib.KmcScan(ctx, K, P, 1, R, lut)
    sc.set_count_range(1, 255)
    hist.zero()
    over.zero()
    sc.kmer_stats(d.ptr, 0, R, hist.ptr, over.ptr)   # warm-up
    ctx.sync()
    ms = []
    for _ in range(REPS):
        timer.start()
        sc.kmer_stats(d.ptr, 0, R, hist.ptr, over.ptr)
        timer.stop()
        ctx.sync()
        ms.append(timer.elapsed_ms())
    h = hist.download(np.uint64, bins)
    assert int(h.sum()) == R * (REPS + 1) and int(over.download(np.uint64, 1)[0]) == 0
    nz = int(np.count_nonzero(h))
    if name == "one-bin":
        assert nz == 1 and int(np.nonzero(h)[0][0]) // ncomp == 1   # count 1
    best = min(ms)
    print(f"{name:8s} {R} records: {' '.join('%.2f' % x for x in ms)} ms per pass, best {best:.2f} ms = {R / (best / 1e3):.3e} records/s, {nz} non-zero bins")
    sc.close()
    d.free()
timer.close()
ctx.close()
