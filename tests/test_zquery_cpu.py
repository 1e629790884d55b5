"""CPU-only: tests/zquery_ref.py (the judge of `kmx query --z`) against an example whose windows are written out here, its two roads
against each other, z = 0 against query_ref, the K-positions of short queries and of queries with an N in every place, and the new
symbols of the C ABI as the header and the binding name them."""
import os
import re
import numpy as np

import orc
import query_ref as qr
import zquery_ref as zr
from test_query_cpu import K, M, N, P, SEQ, W, WORKED, worked_matrices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# z = 2 over test_query_cpu's worked sequence (k = 8: 10-mers).  The N at base 19 leaves the k-mer positions 0 .. 11 and 20 .. 32; a
# window needs the positions j, j + 1, j + 2, so the K-positions are 0 .. 9 and 20 .. 30: 21 of them.
# j: (the bits 0 .. 2 of the rows at j, j + 1, j + 2 as WORKED lists them, their AND)
WINDOWS = {
    0: ((0b001, 0b101, 0b010), 0b000), 1: ((0b101, 0b010, 0b101), 0b000), 2: ((0b010, 0b101, 0b001), 0b000), 3: ((0b101, 0b001, 0b110), 0b000),
    4: ((0b001, 0b110, 0b011), 0b000), 5: ((0b110, 0b011, 0b110), 0b010), 6: ((0b011, 0b110, 0b001), 0b000), 7: ((0b110, 0b001, 0b111), 0b000),
    8: ((0b001, 0b111, 0b101), 0b001), 9: ((0b111, 0b101, 0b100), 0b100),
    20: ((0b011, 0b101, 0b000), 0b000), 21: ((0b101, 0b000, 0b110), 0b000), 22: ((0b000, 0b110, 0b111), 0b000), 23: ((0b110, 0b111, 0b110), 0b110),
    24: ((0b111, 0b110, 0b100), 0b100), 25: ((0b110, 0b100, 0b111), 0b100), 26: ((0b100, 0b111, 0b000), 0b000), 27: ((0b111, 0b000, 0b000), 0b000),
    28: ((0b000, 0b000, 0b001), 0b000), 29: ((0b000, 0b001, 0b001), 0b000), 30: ((0b001, 0b001, 0b001), 0b001),
}


def test_worked_example():
    rep, mats = orc.repart_static(M, P), worked_matrices()
    bits = {w[0]: w[5] for w in WORKED}
    part = {w[0]: w[3] for w in WORKED}
    up = SEQ.upper()
    assert sorted(WINDOWS) == [j for j in range(len(SEQ) - 10 + 1) if "N" not in up[j:j + 10]]
    for j, (rows, both) in WINDOWS.items():
        assert rows == tuple(bits[j + t] for t in range(3)) and both == rows[0] & rows[1] & rows[2], j
    for road in (zr.zquery_expected, zr.zquery_expected_np):
        n, hits = road([SEQ], K, 2, M, rep, W, N, mats)
        assert n[0] == len(WINDOWS) == 21
        assert list(hits[0]) == [sum((w[1] >> i) & 1 for w in WINDOWS.values()) for i in range(N)] == [2, 2, 4]
        # partition 1 is in no call: its k-mers (positions 10, 11 and 20 .. 27) have rows of zeros; their windows still count
        n, hits = road([SEQ], K, 2, M, rep, W, N, [mats[0], None])
        alive = [both for j, (_, both) in WINDOWS.items() if all(part[j + t] == 0 for t in range(3))]
        assert n[0] == 21 and list(hits[0]) == [sum((b >> i) & 1 for b in alive) for i in range(N)] == [1, 1, 0]


def test_the_two_roads_agree():
    """Python integers against numpy: another canonical form, another XXH64, another minimizer walk, another way to slide the window"""
    for k, m in ((12, 8), (31, 10), (32, 10), (33, 10), (64, 10), (96, 10), (97, 10), (127, 10)):
        mats, rep = qr.synth_index(k, 65, 4099, 4, k, m, 0.8, pad_ones=True)
        reads = qr.random_reads(k, 6, 200) + ["N" + "ACGT" * 40 + "n" + "acgtt" * 40, "", "ACG", "A" * 150] + qr.random_reads(k + 1, 3, 160, "ACGTNacgt" + "ACGT" * 8)
        for z in (0, 1, 3, 8):
            for mm in (mats, [mt if p % 2 else None for p, mt in enumerate(mats)]):
                a = zr.zquery_expected(reads, k, z, m, rep, 4099, 65, mm)
                b = zr.zquery_expected_np(reads, k, z, m, rep, 4099, 65, mm)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, z)
                assert a[1].any() and (a[1].max(axis=1) < np.maximum(a[0], 1)).any()      # some windows hit, not all of them


def test_z_zero_is_the_plain_query():
    for k, m in ((12, 8), (31, 10), (64, 10)):
        mats, rep = qr.synth_index(k + 1, 33, 257, 3, k, m, 0.5, pad_ones=True)
        reads = qr.random_reads(k, 5, 150) + ["", "acgtn" * 30, "A" * 90]
        want = qr.query_expected(reads, k, m, rep, 257, 33, mats)
        for road in (zr.zquery_expected, zr.zquery_expected_np):
            got = road(reads, k, 0, m, rep, 257, 33, mats)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k


def test_k_positions():
    """queries of length K - 1, K and K + 1, and a K + 4-base query with an N in every place"""
    k, z, m = 12, 3, 8
    Kz = k + z
    mats, rep = qr.synth_index(4, 5, 101, 2, k, m, 0.8)
    s = qr.random_reads(1, 1, Kz + 4)[0]
    reads = [s[:Kz - 1], s[:Kz], s[:Kz + 1]] + [s[:i] + "N" + s[i + 1:] for i in range(len(s))]
    # an N at base i of L = K + 4 bases leaves the windows in front of it (i - K + 1 of them) and behind it (L - i - K)
    want = [0, 1, 2] + [max(0, i - Kz + 1) + max(0, len(s) - i - Kz) for i in range(len(s))]
    assert want[3] == 4 and want[-1] == 4 and 0 in want[3:]
    for road in (zr.zquery_expected, zr.zquery_expected_np):
        n, hits = road(reads, k, z, m, rep, 101, 5, mats)
        assert list(n) == want
        assert not hits[0].any() and (hits <= n[:, None]).all()


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    declared = set(re.findall(r"\b(kmx_zquery_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"ZQUERY_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no ZQUERY_EXPORTS"
    bound = set(re.findall(r'"(kmx_zquery_\w+)"', listed.group(1)))
    want = {"kmx_zquery_bits_bytes", "kmx_zquery_dev", "kmx_zquery_host"} | {"kmx_zquery_result_" + s for s in
            ("wait", "n_seqs", "copy_kmers", "copy_hits", "hits_dev", "bits_dev", "kernel_ms", "algo_bytes", "free")}
    assert declared == want == bound
    # the binding's structure has the header's fields in the header's order; kmx_query_task is as it was
    def fields(name):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr, re.S).group(1), flags=re.S)
        return [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    struct_src = re.search(r"class KmxZqueryTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert fields("kmx_zquery_task") == re.findall(r'\("(\w+)"', struct_src)
    assert fields("kmx_zquery_task") == fields("kmx_query_task")[:-1] + ["z", "last", "bits", "hits"]
    assert fields("kmx_query_task") == ["bases", "offsets", "n_seqs", "kmer_size", "minim_size", "repart", "nb_parts", "n_cols", "window", "rows", "hits"]


def test_library_exports_the_symbols():
    """the built library has them (kmx_version is unchanged), and the table's size is the header's formula"""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert lib.kmx_version() == 2
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    for name in re.findall(r'"(kmx_zquery_\w+)"', re.search(r"ZQUERY_EXPORTS = \[(.*?)\]", src, re.S).group(1)):
        assert hasattr(lib, name), name
    lib.kmx_zquery_bits_bytes.restype = ctypes.c_uint64
    lib.kmx_zquery_bits_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    for n_cols, pitch in ((1, 4), (32, 4), (33, 8), (64, 8), (65, 12), (100, 16), (2500, 316)):
        assert lib.kmx_zquery_bits_bytes(1000, n_cols) == 1000 * pitch == 1000 * 4 * -(-(-(-n_cols // 8)) // 4)
    assert lib.kmx_zquery_bits_bytes(2 ** 32 - 1, 2500) == (2 ** 32 - 1) * 316
