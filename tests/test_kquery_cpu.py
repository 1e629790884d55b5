"""CPU-only: tests/kquery_ref.py (the judge of `kmx query --kmer-index`) against an example worked by hand, the two roads of the
restatement against each other, the text of the driver's three formats produced from tables, and the new symbols of the C ABI as the
header and the binding name them."""
import os
import re
import numpy as np

import orc
import kquery_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, P, N = 8, 4, 2, 3
SEQ = "ACGTTGCAACGTTGCAtagNCCGATAGGCTTACGTTGCAG"      # tests/test_query_cpu.py's worked sequence: 25 valid positions


def test_worked_example():
    """the canonical k-mers of test_query_cpu.WORKED, a matrix of three of them and two near misses"""
    from test_query_cpu import WORKED
    rep = orc.repart_static(M, P)
    at = kr.places([SEQ], K, M, rep)[0]
    assert [(p, orc.kmer_to_string(np.array([c], np.uint64), K)) for p, c in at] == [(w[3], w[2]) for w in WORKED]
    val = lambda s: int(orc.kmer_from_string(s)[0])
    # partition 0: ACGTTGCA (positions 0, 4, 8, 31), CGTTGCAA (1, 3), and AACGTTGC + 1 (a near miss of positions 5 and 7);
    # partition 1: CGATAGGC (21) and TATGCAAC - 1 (a near miss of position 10)
    k0 = sorted([val("ACGTTGCA"), val("CGTTGCAA"), val("AACGTTGC") + 1])
    k1 = sorted([val("CGATAGGC"), val("TATGCAAC") - 1])
    counts = lambda keys: np.array([[7 * (i + 1), 0, 0xFFFFFFFF] for i in range(len(keys))], np.uint32).view(np.uint8).reshape(len(keys), 12)
    mats = [kr.make_body(k0, counts(k0), K), kr.make_body(k1, counts(k1), K)]
    n, hits, sums = kr.kquery_expected([SEQ], K, M, rep, N, kr.MODE_COUNT, mats)
    assert n[0] == 25
    # six positions meet a row of partition 0, one a row of partition 1; column 1 is zero in every row: found, no hit
    assert list(hits[0]) == [7, 0, 7]
    r0 = {key: i for i, key in enumerate(k0)}
    want0 = 4 * 7 * (r0[val("ACGTTGCA")] + 1) + 2 * 7 * (r0[val("CGTTGCAA")] + 1) + 7 * (k1.index(val("CGATAGGC")) + 1)
    assert list(sums[0]) == [want0, 0, 7 * 0xFFFFFFFF] and sums[0, 2] > 2 ** 32
    # PA rows with every padding bit set: bits 0 .. 2 of row r = r + 1
    bits = lambda keys: np.array([[(i + 1) | 0xF8] for i in range(len(keys))], np.uint8)
    pm = [kr.make_body(k0, bits(k0), K), kr.make_body(k1, bits(k1), K)]
    n, hits, sums = kr.kquery_expected([SEQ], K, M, rep, N, kr.MODE_PA, pm)
    rows = [r0[val("ACGTTGCA")] + 1] * 4 + [r0[val("CGTTGCAA")] + 1] * 2 + [k1.index(val("CGATAGGC")) + 1]
    assert n[0] == 25 and list(hits[0]) == [sum((r >> i) & 1 for r in rows) for i in range(3)] and not sums.any()
    # a partition that is not part of the call
    n, hits, _ = kr.kquery_expected([SEQ], K, M, rep, N, kr.MODE_PA, [pm[0], None])
    assert n[0] == 25 and list(hits[0]) == [sum((r >> i) & 1 for r in rows[:6]) for i in range(3)]


def test_queries_without_a_kmer_are_reported():
    rep = orc.repart_static(M, P)
    mats, _ = kr.synth_kindex(1, N, P, K, M, kr.MODE_COUNT, [SEQ], 1.0, near=0.0)
    n, hits, sums = kr.kquery_expected(["", "ACGTACG", "ACGNACGTNACGTACN", SEQ], K, M, rep, N, kr.MODE_COUNT, mats)
    assert list(n) == [0, 0, 0, 25] and not hits[:3].any() and not sums[:3].any()
    assert (hits[3] == 25).all()      # frac 1, no near misses, no zero counts: every k-mer of the read is a row


def test_the_two_roads_agree():
    """the loop over positions and the road through the CPU checker's split and count (what the long GPU cases are judged by)"""
    for k, m in ((12, 8), (31, 10), (33, 10), (64, 10), (96, 10), (127, 10)):
        reads = ["A" * 40 + r for r in kr.random_reads(k, 6, 200)] + ["N" + "ACGT" * 40 + "n" + "acgtt" * 40, "", "ACG", "A" * 150]
        for mode in (kr.MODE_COUNT, kr.MODE_PA):
            mats, rep = kr.synth_kindex(k, 9, 4, k, m, mode, reads, 0.6, near=0.3, pad_ones=True, zeros=0.2, maxed=0.1)
            a = kr.kquery_expected(reads, k, m, rep, 9, mode, mats)
            b = kr.kquery_expected_bulk(reads, k, m, rep, 9, mode, mats)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, mode)
            assert a[1].any() and (a[1].sum(axis=1) < a[0].astype(np.uint64) * 9).any()      # some found, some not
            none = [mt if p % 2 else None for p, mt in enumerate(mats)]
            a, b = kr.kquery_expected(reads, k, m, rep, 9, mode, none), kr.kquery_expected_bulk(reads, k, m, rep, 9, mode, none)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, mode)


def test_near_misses_are_in_the_index():
    """synth_kindex puts key - 1 / key + 1 in place of a share of the keys: such rows are no k-mer of the reads"""
    reads = ["A" * 40 + r for r in kr.random_reads(3, 20, 110)]
    rep = orc.repart_static(10, 4)
    own = kr.read_keys(reads, 64, 10, rep, 4)
    mats, _ = kr.synth_kindex(5, 3, 4, 64, 10, kr.MODE_PA, reads, 1.0, near=0.5, keys=own)
    misses = 0
    for p, mt in enumerate(mats):
        keys = [kr._value(row) for row in kr.split_matrix(mt, 64, 3, kr.MODE_PA)[0]]
        assert keys == sorted(set(keys))
        missing = set(keys) - set(own[p])
        assert all(key - 1 in own[p] or key + 1 in own[p] for key in missing)
        misses += len(missing)
    assert misses > 100


def test_text_formats():
    names, ids = ["q1", "empty", "q3"], ["D1", "D2", "D3"]
    n = np.array([10, 0, 3], np.uint32)
    hits = np.array([[7, 6, 10], [0, 0, 0], [3, 2, 0]], np.uint32)
    sums = np.array([[70, 6, 2 ** 40 + 1], [0, 0, 0], [3, 2 ** 33, 0]], np.uint64)
    assert kr.format_matrix(names, ids, n, hits) == "query\tn_kmers\tD1\tD2\tD3\nq1\t10\t7\t6\t10\nempty\t0\t0\t0\t0\nq3\t3\t3\t2\t0\n"
    assert kr.format_list(names, ids, n, hits) == "q1\tD1\t7\t10\nq1\tD3\t10\t10\nq3\tD1\t3\t3\n"
    assert kr.format_sums(names, ids, n, sums) == f"query\tn_kmers\tD1\tD2\tD3\nq1\t10\t70\t6\t{2 ** 40 + 1}\nempty\t0\t0\t0\t0\nq3\t3\t3\t{2 ** 33}\t0\n"


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_kquery_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"KQUERY_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no KQUERY_EXPORTS"
    bound = set(re.findall(r'"(kmx_kquery_\w+)"', listed.group(1)))
    want = {"kmx_kquery_dev", "kmx_kquery_host"} | {"kmx_kquery_result_" + s for s in
            ("wait", "n_seqs", "copy_kmers", "copy_hits", "copy_sums", "hits_dev", "sums_dev", "kernel_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert re.search(r"\bKMX_VERSION = 2\b", src)
    for f in ("key_words", "mode", "n_rows", "sums", "want_sums"):
        assert re.search(r"typedef struct \{[^}]*\b" + f + r";[^}]*\} kmx_kquery_task;", hdr, re.S), f
    assert "window" not in re.search(r"typedef struct \{([^}]*)\} kmx_kquery_task;", hdr, re.S).group(1)
    # the binding's structure has the header's fields in the header's order
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_kquery_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    struct_src = re.search(r"class KmxKqueryTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    assert c_fields == ["bases", "offsets", "n_seqs", "kmer_size", "minim_size", "repart", "nb_parts", "n_cols", "key_words", "mode", "n_rows",
                        "rows", "hits", "sums", "want_sums"]


def test_library_exports_the_symbols():
    """the built library has them (and kmx_version is unchanged)"""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert lib.kmx_version() == 2
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    for name in re.findall(r'"(kmx_kquery_\w+)"', re.search(r"KQUERY_EXPORTS = \[(.*?)\]", src, re.S).group(1)):
        assert hasattr(lib, name), name
