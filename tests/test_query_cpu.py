"""CPU-only: tests/query_ref.py (the judge of `kmx query`) against an example worked by hand, the two roads of the restatement
against each other, and the text of the driver's two formats produced from a table."""
import numpy as np

import orc
import query_ref as qr

K, M, P, W, N = 8, 4, 2, 11, 3
#      0         1         2         3
#      0123456789012345678901234567890123456789
SEQ = "ACGTTGCAACGTTGCAtagNCCGATAGGCTTACGTTGCAG"      # 40 bases: a repeat, lower case, one N

# position, its k-mer (upper case), the canonical form (min(forward, reverse complement) with A < C < T < G, the first base the top
# digit), the partition (repart[least m-mer value]), the row (XXH64 of the canonical k-mer's one word % 11), the row's bits 0 .. 2.
# Positions 12 .. 19 hold the N at base 19: no k-mer ("every position j whose k bases are all ACGT").
WORKED = [
    (0, "ACGTTGCA", "ACGTTGCA", 0, 8, 0b001), (1, "CGTTGCAA", "CGTTGCAA", 0, 4, 0b101), (2, "GTTGCAAC", "GTTGCAAC", 0, 5, 0b010),
    (3, "TTGCAACG", "CGTTGCAA", 0, 4, 0b101),      # the reverse complement of position 1's k-mer: the same row ("c = canonical k-mer")
    (4, "TGCAACGT", "ACGTTGCA", 0, 8, 0b001), (5, "GCAACGTT", "AACGTTGC", 0, 1, 0b110), (6, "CAACGTTG", "CAACGTTG", 0, 10, 0b011),
    (7, "AACGTTGC", "AACGTTGC", 0, 1, 0b110),
    (8, "ACGTTGCA", "ACGTTGCA", 0, 8, 0b001),      # position 0's k-mer again: counted again ("every occurrence counts")
    (9, "CGTTGCAT", "ATGCAACG", 0, 6, 0b111),      # bases 16 .. 18 are lower case ("in either letter case")
    (10, "GTTGCATA", "TATGCAAC", 1, 5, 0b101), (11, "TTGCATAG", "CTATGCAA", 1, 0, 0b100),
    (20, "CCGATAGG", "CCTATCGG", 1, 3, 0b011), (21, "CGATAGGC", "CGATAGGC", 1, 5, 0b101),
    (22, "GATAGGCT", "AGCCTATC", 1, 4, 0b000),     # a row without a bit below N: counted in n_kmers, no hit (its padding bits are set)
    (23, "ATAGGCTT", "AAGCCTAT", 1, 10, 0b110), (24, "TAGGCTTA", "TAAGCCTA", 1, 7, 0b111), (25, "AGGCTTAC", "AGGCTTAC", 1, 2, 0b110),
    (26, "GGCTTACG", "CGTAAGCC", 1, 8, 0b100), (27, "GCTTACGT", "ACGTAAGC", 1, 7, 0b111), (28, "CTTACGTT", "AACGTAAG", 0, 3, 0b000),
    (29, "TTACGTTG", "CAACGTAA", 0, 3, 0b000), (30, "TACGTTGC", "TACGTTGC", 0, 0, 0b001), (31, "ACGTTGCA", "ACGTTGCA", 0, 8, 0b001),
    (32, "CGTTGCAG", "CTGCAACG", 0, 0, 0b001),
]


def worked_matrices():
    """row h of partition p: bits 0 .. 2 = (5 h + 3 p + 1) & 7, every padding bit set"""
    return [np.array([[((h * 5 + p * 3 + 1) & 7) | 0xF8] for h in range(W)], np.uint8) for p in range(P)]


def test_worked_example():
    lut, rep, mats = orc.minimizer_lut(M), orc.repart_static(M, P), worked_matrices()
    order = {c: i for i, c in enumerate("ACTG")}
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    up = SEQ.upper()
    assert [w[0] for w in WORKED] == [j for j in range(len(SEQ) - K + 1) if "N" not in up[j:j + K]]
    for j, kmer, canon, p, h, bits in WORKED:
        assert up[j:j + K] == kmer
        rc = "".join(comp[c] for c in reversed(kmer))
        assert canon == min(kmer, rc, key=lambda s: [order[c] for c in s])
        assert qr.kmer_address(kmer, K, M, lut, rep, W) == (p, h), (j, kmer)
        assert int(mats[p][h][0]) & 7 == bits
    n, hits = qr.query_expected([SEQ], K, M, rep, W, N, mats, lut)
    assert n[0] == len(WORKED) == 25
    assert list(hits[0]) == [sum((w[5] >> i) & 1 for w in WORKED) for i in range(N)] == [15, 10, 13]
    # a partition that is not part of the call: its k-mers count in n_kmers, its rows add nothing
    n0, h0 = qr.query_expected([SEQ], K, M, rep, W, N, [mats[0], None], lut)
    assert n0[0] == 25 and list(h0[0]) == [sum((w[5] >> i) & 1 for w in WORKED if w[3] == 0) for i in range(N)]


def test_queries_without_a_kmer_are_reported():
    rep, mats = orc.repart_static(M, P), worked_matrices()
    n, hits = qr.query_expected(["", "ACGTACG", "ACGNACGTNACGTACN", SEQ], K, M, rep, W, N, mats)
    assert list(n) == [0, 0, 0, 25] and not hits[:3].any()


def test_the_two_roads_agree():
    """the loop over positions and the road through the CPU checker's split and count (what the long GPU cases are judged by)"""
    for k, m in ((12, 8), (31, 10), (33, 10), (64, 10), (96, 10), (127, 10)):
        mats, rep = qr.synth_index(k, 65, 4099, 4, k, m, 0.3, pad_ones=True)
        reads = qr.random_reads(k, 6, 200) + ["N" + "ACGT" * 40 + "n" + "acgtt" * 40, "", "ACG", "A" * 150]
        a = qr.query_expected(reads, k, m, rep, 4099, 65, mats)
        b = qr.query_expected_bulk(reads, k, m, rep, 4099, 65, mats)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k


def test_text_formats():
    names, ids = ["q1", "empty", "q3"], ["D1", "D2", "D3"]
    n = np.array([10, 0, 3], np.uint32)
    hits = np.array([[7, 6, 10], [0, 0, 0], [3, 2, 0]], np.uint32)
    assert qr.format_matrix(names, ids, n, hits) == "query\tn_kmers\tD1\tD2\tD3\nq1\t10\t7\t6\t10\nempty\t0\t0\t0\t0\nq3\t3\t3\t2\t0\n"
    # 7 == 0.7 * 10 exactly as doubles: kept; 6 is not; a query without k-mers has no line; 2 < 0.7 * 3 = 2.1
    assert qr.format_list(names, ids, n, hits) == "q1\tD1\t7\t10\nq1\tD3\t10\t10\nq3\tD1\t3\t3\n"
    assert qr.format_list(names, ids, n, hits, 0.0) == "".join(f"{q}\t{s}\t{h}\t{k}\n" for q, k, row in (("q1", 10, hits[0]), ("q3", 3, hits[2])) for s, h in zip(ids, row))
    assert qr.format_list(names, ids, n, hits, 1.0) == "q1\tD3\t10\t10\nq3\tD1\t3\t3\n"
    assert float(7) >= 0.7 * float(10)
