"""The k-mer table checkpoint file and its manifest, without a GPU: bt_table_file_info on files written here by a small writer of the documented
format (include/btgpu.h: bt_table_save) — the fields come back, and every kind of damage is refused with a message that names it — and the manifest
builder of the executable (host/TableCheckpoint.hpp) — equal inputs give equal text, a changed input changes its own line."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

MAGIC = b"BTAMDKTBL1"


def record_bytes(num_samples):
    return 20 + ((num_samples + 3) & ~3)


def write_checkpoint(path, k, num_samples, records, manifest, chunk_records):
    """records: (n, record_bytes) uint8.  header | chunks | trailer, all little endian (bt_table_file.hpp)"""
    rb = record_bytes(num_samples)
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, rb)
    m = manifest.encode()
    head = MAGIC + struct.pack("<IIIIQQI", 1, k, num_samples, rb, len(records), chunk_records, len(m)) + m
    out = head + struct.pack("<I", zlib.crc32(head))
    for i in range(0, len(records), chunk_records):
        body = struct.pack("<Q", len(records[i:i + chunk_records])) + records[i:i + chunk_records].tobytes()
        out += b"CHNK" + body + struct.pack("<I", zlib.crc32(body))
    count = struct.pack("<Q", len(records))
    out += b"TEND" + count + struct.pack("<I", zlib.crc32(count))
    with open(path, "wb") as f:
        f.write(out)
    return out


MANIFEST = "k=55\nsamples=3\nsample.0.name=a\n"


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    rng = np.random.default_rng(5)
    records = rng.integers(0, 256, (700, record_bytes(3)), dtype=np.uint8)
    path = str(d / "table.ckpt")
    return d, path, write_checkpoint(path, 55, 3, records, MANIFEST, 256)   # chunks of 256, 256 and 188 records


def test_file_info_returns_the_fields(good):
    from bayestyper_amd import lib

    _, path, _ = good
    assert lib.table_file_info(path) == {"k": 55, "num_samples": 3, "num_records": 700, "manifest": MANIFEST}


def test_file_info_of_an_empty_table(tmp_path):
    from bayestyper_amd import lib

    path = str(tmp_path / "empty.ckpt")
    write_checkpoint(path, 31, 10, np.zeros((0, record_bytes(10)), np.uint8), "", 1024)
    assert lib.table_file_info(path) == {"k": 31, "num_samples": 10, "num_records": 0, "manifest": ""}


def _header_len():
    return len(MAGIC) + 4 * 4 + 8 + 8 + 4 + len(MANIFEST) + 4


def _flip(data, at):
    return data[:at] + bytes([data[at] ^ 0x40]) + data[at + 1:]


# (name, damage, what the message must name)
DAMAGE = [
    ("header-field", lambda b: _flip(b, len(MAGIC) + 5), "header CRC mismatch"),        # a byte of k
    ("header-manifest", lambda b: _flip(b, _header_len() - 8), "header CRC mismatch"),
    ("header-magic", lambda b: _flip(b, 3), "bad magic"),
    ("payload-first-chunk", lambda b: _flip(b, _header_len() + 12 + 1000), "chunk CRC mismatch"),
    ("payload-last-chunk", lambda b: _flip(b, len(b) - 16 - 4 - 50), "chunk CRC mismatch"),
    ("missing-trailer", lambda b: b[:-16], "missing trailer"),
    ("half-a-trailer", lambda b: b[:-7], "trailer"),
    ("truncated-in-a-chunk", lambda b: b[:_header_len() + 12 + 256 * record_bytes(3) + 4 + 12 + 3000], "truncated in a chunk"),
    ("truncated-header", lambda b: b[:20], "truncated header"),
]


@pytest.mark.parametrize("damage,names", [d[1:] for d in DAMAGE], ids=[d[0] for d in DAMAGE])
def test_damage_is_refused_by_name(good, damage, names):
    from bayestyper_amd import lib

    d, _, data = good
    path = str(d / "damaged.ckpt")
    with open(path, "wb") as f:
        f.write(damage(data))
    with pytest.raises(lib.BtError, match=names) as e:
        lib.table_file_info(path)
    assert "damaged.ckpt" in str(e.value)


def test_a_missing_file_is_an_error():
    from bayestyper_amd import lib

    with pytest.raises(lib.BtError, match="cannot open"):
        lib.table_file_info("/nonexistent/table.ckpt")


def _manifest(names, suf_bytes, present=(1, 1, 1)):
    from bayestyper_amd.host import dll

    S = len(names)
    u8, u32, u64 = (lambda v: np.ascontiguousarray(v, np.uint8)), (lambda v: np.ascontiguousarray(v, np.uint32)), (lambda v: np.ascontiguousarray(v, np.uint64))
    arrays = [u8(present), u64([1000 + s for s in range(S)]), u64(suf_bytes), u32([1] * S), u32([2] * S), u64([255] * S)]
    files = [u64([10, 20, 30]), u32([0xDEADBEEF, 1, 2])]
    chroms = [u64([70000, 500]), u8([0, 1]), u8([2, 0]), u8([1, 0])]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fn = dll.bth_table_checkpoint_manifest
    fn.restype = C.c_ulonglong
    fn.argtypes = [C.c_uint, C.c_uint, C.c_char_p] + [C.c_void_p] * 6 + [C.c_uint, C.c_char_p] + [C.c_void_p] * 2 + [C.c_uint, C.c_char_p] + [C.c_void_p] * 4 + [C.c_char_p, C.c_ulonglong]
    out = C.create_string_buffer(1 << 16)
    n = fn(55, S, "\t".join(names).encode(), *[p(a) for a in arrays], 3, b"variant_clusters.bin\tparameter_kmers.fa.gz\tintercluster_regions.txt.gz", *[p(a) for a in files], 2,
           b"chr1\tdecoy1", *[p(a) for a in chroms], out, 1 << 16)
    assert 0 < n == len(out.value)
    return out.value.decode()


def test_manifest_is_a_function_of_its_inputs():
    names, sizes = ["s1", "s2", "s3"], [13004, 13017, 13030]
    a = _manifest(names, sizes)
    assert a == _manifest(names, sizes)
    lines = a.split("\n")
    assert lines[:3] == ["k=55", "samples=3", "sample.0.name=s1"] and all("=" in ln for ln in lines[:-1]) and lines[-1] == ""
    assert "file.variant_clusters.bin=bytes:10 crc32:deadbeef" in lines and "chromosome.chr1=length:70000 decoy:0 ploidy:2/1" in lines
    # nothing that does not determine the table: no seed, no Gibbs option, no gender
    assert not any(w in a for w in ("seed", "gibbs", "gender"))
    # one sample's .kmc_suf size changes: exactly that sample's database line differs
    b = _manifest(names, [13004, 13018, 13030]).split("\n")
    assert [i for i in range(len(lines)) if lines[i] != b[i]] == [lines.index("sample.1.name=s2") + 1] and "suf_bytes:13018" in b[lines.index("sample.1.name=s2") + 1]
    # two samples swap places: their lines differ (sample s owns count byte s)
    c = _manifest(["s2", "s1", "s3"], [13017, 13004, 13030]).split("\n")
    assert c != lines and c[2] == "sample.0.name=s2" and lines.index("sample.1.name=s2") != c.index("sample.0.name=s2")
    # a database that is not there reads "absent"
    assert "sample.2.kmc=absent" in _manifest(names, sizes, present=(1, 1, 0)).split("\n")
