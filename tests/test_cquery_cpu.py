"""CPU-only: tests/cquery_ref.py (the judge of `kmx query` over a counting Bloom index) against the rows include/kmx.h works by hand,
its two roads against each other, the w = 1 case against tests/query_ref.py, its unpacker against the oracle's own BFC merge, and the
new symbols of the C ABI as the header and the binding name them."""
import os
import re
import numpy as np
import pytest

import orc
import query_ref as qr
import cquery_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/kmx.h, section "cquery", EXAMPLES: w = 3, N = 3, the third field across the two bytes, every padding bit set
ROWS = [(bytes([0x22, 0xFF]), (1, 0, 5), (1, 0, 16)),
        (bytes([0xED, 0x7F]), (7, 3, 2), (64, 4, 2)),
        (bytes([0x1B, 0xFF]), (0, 6, 7), (0, 32, 64))]


def test_worked_rows():
    for raw, classes, floors in ROWS:
        R = int.from_bytes(raw, "big")
        assert tuple((R >> (16 - (i + 1) * 3)) & 7 for i in range(3)) == classes
        assert tuple(int(x) for x in cr.unpack_classes(np.frombuffer(raw, np.uint8).reshape(1, 2), 3, 3)[0]) == classes
        assert tuple(cr.floor_of(v) for v in classes) == floors
        for pad in (False, True):
            packed = cr.pack_classes(np.array([classes]), 3, pad_ones=pad)
            assert packed.shape == (1, 2) and packed[0, 0] == raw[0] and (packed[0, 1] & 0x80) == (raw[1] & 0x80)
            assert (packed[0, 1] & 0x7F) == (0x7F if pad else 0)
    # w = 8: a byte of ones is class 255, clamped
    assert int(cr.unpack_classes(np.array([[0xFF]], np.uint8), 1, 8)[0, 0]) == 255 and cr.floor_of(255) == 2 ** 31


@pytest.mark.parametrize("road", [cr.cquery_expected, cr.cquery_expected_np])
def test_worked_query(road):
    """a query of three valid positions that meet the three rows"""
    k, m, P, W, N, w = 8, 4, 2, 1009, 3, 3
    seq = "ACGTTGCAAC"
    rep = orc.repart_static(m, P)
    lut = orc.minimizer_lut(m)
    at = [qr.kmer_address(seq[j:j + k], k, m, lut, rep, W) for j in range(3)]
    assert len(set(at)) == 3
    mats = [np.zeros((W, 2), np.uint8) for _ in range(P)]
    for (p, h), (raw, _, _) in zip(at, ROWS):
        mats[p][h] = np.frombuffer(raw, np.uint8)
    for mc, want in ((1, [2, 2, 3]), (4, [1, 1, 2]), (7, [1, 0, 1])):
        n, hits, sums = road([seq, "ACGTNACGTACG"], k, m, rep, W, N, mats, w, mc)
        assert list(n) == [3, 0] and list(hits[0]) == want and [int(x) for x in sums[0]] == [65, 36, 82]
        assert not hits[1].any() and not sums[1].any()
    # a partition that is not part of the call adds nothing and still counts in n_kmers
    only = [mats[0], None]
    n, hits, sums = road([seq], k, m, rep, W, N, only, w, 1)
    keep = [r for (p, _), r in zip(at, ROWS) if p == 0]
    assert n[0] == 3 and [int(x) for x in sums[0]] == [sum(r[2][i] for r in keep) for i in range(3)]


def test_floor_of():
    assert [cr.floor_of(v) for v in (0, 1, 32, 33, 255)] == [0, 1, 2 ** 31, 2 ** 31, 2 ** 31]
    assert all(cr.floor_of(orc.to_n_b(c, 6)) <= c for c in (1, 2, 3, 255, 256, 2 ** 32 - 1))      # a lower bound of the count it stands for
    assert all(cr.floor_of(v) == 1 << (v - 1) for v in range(1, 33))


def reads_for(k):
    return ["A" * 40 + qr.random_reads(k, 1, 160)[0], "N" + "ACGT" * 40 + "n" + "acgtt" * 40, "", "ACG", qr.random_reads(k + 1, 1, 150)[0].lower(),
            qr.random_reads(k + 2, 1, k - 1)[0]]


CASES = [(k, w, (1, 7, 8, 9, 65)[(i + w) % 5]) for i, k in enumerate((12, 31, 32, 33, 64, 127)) for w in range(1, 9)] + \
        [(31, w, N) for w in range(1, 9) for N in (1, 7, 8, 9, 65)]


@pytest.mark.parametrize("k,w,N", CASES)
def test_the_two_roads_agree(k, w, N):
    """the loop over positions and the road through the CPU checker's split and count, every padding bit set: all partitions with
    min_class 1, half of them with the top class"""
    m, P, W = (8 if k == 12 else 10), 4, 509
    reads = reads_for(k)
    mats, rep = cr.synth_index_bfc(1000 * k + 10 * N + w, N, W, P, k, m, w, pad_ones=True)
    top = (1 << w) - 1
    a = cr.cquery_expected(reads, k, m, rep, W, N, mats, w, 1)
    b = cr.cquery_expected_np(reads, k, m, rep, W, N, mats, w, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0][0] == 200 - k + 1 and a[0][2] == 0 and a[0][3] == 0 and a[0][5] == 0 and a[0][4] == 150 - k + 1
    assert a[2].any() and (a[1] <= a[0][:, None]).all()
    half = [mt if p % 2 else None for p, mt in enumerate(mats)]
    c = cr.cquery_expected(reads, k, m, rep, W, N, half, w, top)
    d = cr.cquery_expected_np(reads, k, m, rep, W, N, half, w, top)
    assert all(np.array_equal(x, y) for x, y in zip(c, d))
    assert np.array_equal(c[0], a[0]) and (c[2] <= a[2]).all() and (c[1] <= a[1]).all()


def test_one_bit_is_the_bloom_query():
    """w = 1, min_class 1: the hits of query_ref on the same body with every byte's bits reversed (its columns count from bit 0), and
    the sums are the hits (floor_of(1) = 1)"""
    k, m, P, W, N = 31, 10, 4, 509, 13
    reads = reads_for(k)
    mats, rep = cr.synth_index_bfc(3, N, W, P, k, m, 1, pad_ones=True)
    rev = [np.packbits(np.unpackbits(mt, axis=1, bitorder="big"), axis=1, bitorder="little") for mt in mats]
    n, hits, sums = cr.cquery_expected(reads, k, m, rep, W, N, mats, 1, 1)
    en, eh = qr.query_expected(reads, k, m, rep, W, N, rev)
    assert np.array_equal(n, en) and np.array_equal(hits, eh) and np.array_equal(sums, eh.astype(np.uint64)) and eh.any()


@pytest.mark.parametrize("w", [2, 3, 5, 8])
def test_unpacker_reads_what_the_merge_writes(w):
    """the oracle's BFC merge over small lists with counts at every edge: the classes read back are min(bit_length(c), 2^w - 1)"""
    counts = [0, 1, 2, 3, 255, 256, 2 ** 32 - 1]
    N, W, lower = 3, 14, 28      # (partition 2 of a window of 14)
    want = np.array([[counts[(r + 3 * i) % 7] for i in range(N)] for r in range(W)], np.uint64)
    lists = []
    for i in range(N):
        rows = [r for r in range(W) if want[r, i]]
        lists.append((np.array([lower + r for r in rows], np.uint64), np.array([want[r, i] for r in rows], np.uint32)))
    body, rows, _ = orc.merge_matrix(lists, 1, [1] * N, 1, 0, orc.MODE_BFC, lower, lower + W - 1, w)
    nb = (N * w + 7) // 8
    assert len(body) == W * nb
    mat = np.frombuffer(body, np.uint8).reshape(W, nb)
    exp = np.array([[min(int(c).bit_length(), (1 << w) - 1) for c in row] for row in want], np.uint32)
    assert np.array_equal(cr.unpack_classes(mat, N, w), exp)
    for r in range(W):      # and road 1's shifts
        R = int.from_bytes(mat[r].tobytes(), "big")
        assert [(R >> (8 * nb - (i + 1) * w)) & ((1 << w) - 1) for i in range(N)] == list(exp[r])
    assert all(int(exp[r, i]) == orc.to_n_b(int(want[r, i]), w) for r in range(W) for i in range(N))
    assert np.array_equal(cr.pack_classes(exp, w), mat)


def test_text_formats():
    n = np.array([10, 0], np.uint32)
    sums = np.array([[70, 2 ** 40 + 1], [0, 0]], np.uint64)
    assert cr.format_sums(["q1", "empty"], ["D1", "D2"], n, sums) == f"query\tn_kmers\tD1\tD2\nq1\t10\t70\t{2 ** 40 + 1}\nempty\t0\t0\t0\n"


def fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr, re.S).group(1), flags=re.S)
    return [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_cquery_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"CQUERY_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no CQUERY_EXPORTS"
    bound = set(re.findall(r'"(kmx_cquery_\w+)"', listed.group(1)))
    want = {"kmx_cquery_dev", "kmx_cquery_host"} | {"kmx_cquery_result_" + s for s in
            ("wait", "n_seqs", "copy_kmers", "copy_hits", "copy_sums", "hits_dev", "sums_dev", "kernel_ms", "algo_bytes", "free")}
    assert declared == want == bound and len(want) == 12
    assert re.search(r"\bKMX_VERSION = 2\b", src)
    q = fields(hdr, "kmx_query_task")
    assert q == ["bases", "offsets", "n_seqs", "kmer_size", "minim_size", "repart", "nb_parts", "n_cols", "window", "rows", "hits"]      # unchanged
    c = fields(hdr, "kmx_cquery_task")
    assert c == q[:-1] + ["bitw", "min_class", "hits", "sums"]
    struct_src = re.search(r"class KmxCqueryTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c == re.findall(r'\("(\w+)"', struct_src)


def test_library_exports_the_symbols():
    """the built library has them (and kmx_version is unchanged)"""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert lib.kmx_version() == 2
    want = ["kmx_cquery_dev", "kmx_cquery_host"] + ["kmx_cquery_result_" + s for s in
            ("wait", "n_seqs", "copy_kmers", "copy_hits", "copy_sums", "hits_dev", "sums_dev", "kernel_ms", "algo_bytes", "free")]
    for name in want:
        assert hasattr(lib, name), name
