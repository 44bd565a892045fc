"""The tabix index of a BGZF-compressed VCF (bayestyper_amd/host/TabixIndex.cpp, bthost::buildTabixIndex) — ctypes front end."""
import ctypes as C

import numpy as np


def reg2bin(beg, end):
    """the bin of the 0-based half-open interval [beg, end) (min_shift 14, depth 5)"""
    from . import dll

    dll.bth_tabix_reg2bin.restype = C.c_uint32
    dll.bth_tabix_reg2bin.argtypes = [C.c_ulonglong, C.c_ulonglong]
    return dll.bth_tabix_reg2bin(beg, end)


def tabix_index(contigs, block_offsets, lines):
    """contigs: names in file order; block_offsets: [blocks + 1] file offsets (lib.bgzf_save's); lines: rows (contig index, POS, len(REF), offset of the
    line in the uncompressed text, length of the line) in file order -> (the uncompressed .tbi bytes, None), or (None, warning) when no index can be built"""
    from . import dll

    fn = dll.bth_tabix_index
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_char_p, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_char_p, C.c_uint]
    assert all(n and "\t" not in n for n in contigs)
    offs = np.ascontiguousarray(block_offsets, np.uint64)
    table = np.ascontiguousarray(np.asarray(lines, np.uint64).reshape(-1, 5))
    names, err = "\t".join(contigs).encode(), C.create_string_buffer(512)
    need = fn(names, offs.ctypes.data, offs.size, table.ctypes.data, len(table), None, 0, err, 512)
    if need < 0:
        return None, err.value.decode()
    buf = C.create_string_buffer(max(need, 1))
    assert fn(names, offs.ctypes.data, offs.size, table.ctypes.data, len(table), buf, need, err, 512) == need
    return buf.raw[:need], None
