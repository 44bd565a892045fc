"""Shared inputs and restatements of the reads pack tests (test_reads_pack_cpu.py, test_reads_pack_gpu.py): the packed layout in numpy, the canonical text, the
texts every pack test runs over."""
import numpy as np

BLOCK = 128          # positions per block
BLOCK_BYTES = 48     # 8 words of codes, 4 words of validity bits
CPU_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)

_CODE = np.full(256, -1, np.int64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i   # lower case


def np_pack(text):
    """the layout restated: position j of block b -> codes word j // 16 at bits 2 (j % 16), validity word 8 + j // 32 at bit j % 32; padding code 0, invalid"""
    t = np.frombuffer(bytes(text), np.uint8)
    n = len(t)
    blocks = -(-n // BLOCK)
    code = np.zeros(blocks * BLOCK, np.uint64)
    valid = np.zeros(blocks * BLOCK, np.uint64)
    c = _CODE[t]
    code[:n] = np.where(c >= 0, c, 0)
    valid[:n] = c >= 0
    words = np.zeros((blocks, 12), np.uint64)
    j = np.arange(BLOCK, dtype=np.uint64)
    cb, vb = code.reshape(blocks, BLOCK), valid.reshape(blocks, BLOCK)
    for w in range(8):
        sel = slice(16 * w, 16 * w + 16)
        words[:, w] = (cb[:, sel] << (np.uint64(2) * (j[sel] % np.uint64(16)))).sum(axis=1)
    for w in range(4):
        sel = slice(32 * w, 32 * w + 32)
        words[:, 8 + w] = (vb[:, sel] << (j[sel] % np.uint64(32))).sum(axis=1)
    return words.astype("<u4").reshape(-1).view(np.uint8)


def canonical(text):
    """upper-case bases, every other byte a newline"""
    t = np.frombuffer(bytes(text), np.uint8)
    c = _CODE[t]
    return np.where(c >= 0, np.frombuffer(b"ACGT", np.uint8)[np.maximum(c, 0)], 10).astype(np.uint8).tobytes()


def layout_text(rng, n):
    """n bytes that cover all 256 byte values (as far as n allows), lower and mixed case, runs of N and CRLF"""
    parts = [bytes(rng.permutation(256).astype(np.uint8)), b"acgtACGTaCgT", b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN", b"ACGT\r\nacgtn\r\n\r\n",
             np.frombuffer(b"ACGTacgtN\n", np.uint8)[rng.integers(0, 10, size=n + 64)].tobytes()]
    order = rng.permutation(len(parts))
    return b"".join(parts[i] for i in order)[:n] if n else b""


def garbage_padding(packed, positions, rng=None):
    """a copy of the packed reads with every bit at and beyond `positions` of the last block set (rng: random instead)"""
    out = np.array(packed, dtype=np.uint8).view("<u4").copy()
    if positions % BLOCK == 0:
        return out.view(np.uint8)
    base = (positions // BLOCK) * 12
    for j in range(positions % BLOCK, BLOCK):
        bits = 3 if rng is None else int(rng.integers(0, 4))
        out[base + j // 16] |= np.uint32(bits << (2 * (j % 16)))
        if rng is None or rng.integers(0, 2):
            out[base + 8 + j // 32] |= np.uint32(1 << (j % 32))
    return out.view(np.uint8)
