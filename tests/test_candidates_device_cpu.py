"""CPU side of the device-resident candidates: GibbsBatchData::take on a position-only batch (its per-row arrays live in the unit's source on the
device) composes positions and small arrays exactly as take on the full batch followed by dropping the per-row arrays; and libbtgpu.so carries no
library sort any more (the incidence lists are built per row by the library's own kernels)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _take_dump(dll, batch, S, ids, position_only, pos):
    ids = np.ascontiguousarray(ids, np.uint32)
    pos = np.ascontiguousarray(pos, np.uint32)
    args = (C.addressof(batch), S, ids.ctypes.data, len(ids), int(position_only), pos.ctypes.data)
    n = dll.bth_batch_take_dump(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    dll.bth_batch_take_dump(*args, buf, n + 1)
    return buf.value.decode().split("\n")


def test_take_on_a_position_only_batch():
    from bayestyper_amd import synth

    dll = C.CDLL(os.path.join(ROOT, "bayestyper_amd", "libbthost.so"))
    dll.bth_batch_take_dump.restype = C.c_ulonglong
    dll.bth_batch_take_dump.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_char_p, C.c_ulonglong]
    S = 3
    flat = synth.make_mixture(24, S, 5)          # groups of several shapes, nested clusters among them
    G = flat["num_groups"]
    _, batch, keep = synth.to_ctypes(flat)
    rng = np.random.default_rng(1)
    pos = rng.permutation(1000)[:G].astype(np.uint32)      # where each group sits in the (imaginary) source
    for ids in (np.arange(G), np.sort(rng.choice(G, G // 3, replace=False)), np.array([G - 1]), np.arange(3, 11)):
        full = _take_dump(dll, batch, S, ids, False, pos)
        only = _take_dump(dll, batch, S, ids, True, pos)
        assert full[-1] == "" and only[-1] == "" and len(only) == len(full) + 1
        assert only[:-2] == full[:-1]                      # every small array, and no per-row array on either side
        assert full[-2] == "rows: 0 0 0 0 0 0 0 0 0 0"
        assert only[-2] == "source_pos: " + " ".join(str(int(pos[g])) for g in ids)
        assert any(ln.startswith("kmer_off: 0 ") for ln in full) and any(ln.startswith("hap_allele: ") and len(ln) > 13 for ln in full)
    del keep


def test_library_has_no_rocprim_symbol():
    out = subprocess.run(["nm", "-D", "--demangle", os.path.join(ROOT, "bayestyper_amd", "libbtgpu.so")], capture_output=True, text=True, check=True).stdout
    assert "bt_paths_candidates_device" in out and "rocprim" not in out.lower()
