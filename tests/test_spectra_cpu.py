"""CPU-only: tests/spectra_ref.py (the judge of `kmx spectra`) against the example the header works by hand, its two roads against each
other over the sweep, the identities that tie the tables to colsums, pan and dist, `kmx spectra --from-tables` against exact fractions,
the texts of the driver, the new symbols of the C ABI as the header and the binding name them, and the refusals of `kmx spectra` that
come before any device is asked for, on run directories written by hand."""
import ctypes
import math
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import diff_ref as fr
import dist_ref as dr
import pan_ref as pr
import spectra_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = sr.MODE_COUNT, sr.MODE_PA
USAGE_RUN = ("kmx spectra --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
             "[--cap INT=255] [--pairs FILE | --against ID | --all-pairs] [--joint-cap INT=63] [--solid INT=1] [--hist FILE] [--joint FILE] "
             "[--output FILE] [--gpus INT] [--batch-mb INT] [-v]")
USAGE_FROM = "kmx spectra --from-tables HIST_FILE [--joint JOINT_FILE --kmer-size K] [--solid INT] [--output FILE]"


def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def ints(t):
    return None if t is None else np.asarray(t).astype(object).tolist()


def both(body, N, kw, mode, cols=None, cap=255, pairs=None, joint_cap=63):
    """the two roads, equal -> (hist, joint) as lists of integers"""
    h1, j1 = sr.spectra_expected_py(body, N, kw, mode, cols, cap, pairs, joint_cap)
    h2, j2 = sr.spectra_expected_np(body, N, kw, mode, cols, cap, pairs, joint_cap)
    assert h1 == ints(h2) and j1 == ints(j2), (N, kw, mode, cols, cap, pairs, joint_cap)
    return h1, j1


def count_rows(rows, kw=1):
    return b"".join(bytes(range(1, 8 * kw + 1)) + struct.pack(f"<{len(r)}I", *r) for r in rows)


def test_worked_example():
    """the example of include/kmx.h, section spectra, as literals"""
    body = count_rows([(1, 0, 2), (0, 0, 5), (3, 3, 3), (0, 0, 0)])
    hist, joint = both(body, 3, 1, COUNT, cap=2, pairs=[(0, 1), (2, 2)], joint_cap=2)
    assert hist == [[2, 1, 1, 3], [3, 0, 1, 3], [1, 0, 3, 10]]
    assert joint == [[[2, 0, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 0, 0], [0, 0, 3]]]
    assert both(body, 3, 1, COUNT, cols=(2,), cap=2)[0] == [[1, 0, 3, 10]]
    # the column's exact total from its line
    assert [sum(b * h[b] for b in range(2)) + h[3] for h in hist] == [4, 3, 10]
    # the same rows as presence/absence bits, every padding bit set: a bit is a count of 0 or 1
    pa = b"".join(bytes(8) + bytes([b | 0xF8]) for b in (0b101, 0b100, 0b111, 0b000))
    hist, joint = both(pa, 3, 1, PA, cap=2, pairs=[(0, 1), (2, 2)], joint_cap=2)
    assert hist == [[2, 2, 0, 0], [3, 1, 0, 0], [1, 3, 0, 0]]
    assert joint == [[[2, 0, 0], [1, 1, 0], [0, 0, 0]], [[1, 0, 0], [0, 3, 0], [0, 0, 0]]]
    assert both(pa, 3, 1, PA, cap=1)[0] == [[2, 2, 2], [3, 1, 1], [1, 3, 3]]      # C1 = 1: the ones are the last bin, and its volume
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for text in ("(1,0,2)   (0,0,5)   (3,3,3)   (0,0,0)", "hist[0] = (2,1,1, 3)   hist[1] = (3,0,1, 3)   hist[2] = (1,0,3, 10)",
                 "joint[0]: [0][0] = 2, [1][0] = 1, [2][2] = 1;  joint[1]: [0][0] = 1, [2][2] = 3", "With cols = (2) hist is the one line (1,0,3, 10)."):
        assert text in hdr, text


PY_ROAD_CELLS = 400_000      # the Python road walks a case whose rows x (listed columns + pairs) stay below this


def walked(c):
    return c.n_rows * (c.n_use + len(c.pairs)) <= PY_ROAD_CELLS


@pytest.mark.parametrize("name", [c.name for c in sr.gpu_cases() if walked(c)])
def test_the_two_roads_agree_and_the_identities_hold(name):
    """over the sweep the GPU test sends (the cases the Python road can walk in a second; the coverage test says which axes they keep),
    and per case the identities of the header: every line of hist counts the rows; its total is colsums' sum of the column; the rows it
    holds are pan's holders at min_abund 1; the marginals of a joint table are the two columns' histograms folded at C2; the table of
    (x, x) is diagonal; while no count reaches C2 the sum of min(a, b) * joint is dist's sum of minima"""
    c = sr.case(name)
    hist, joint = both(c.body, c.n_cols, c.key_words, c.mode, c.cols, c.cap, c.pairs, c.joint_cap)
    assert hist == ints(c.expected[0]) and joint == ints(c.expected[1])
    check_identities(c, hist, joint)


def check_identities(c, hist, joint):
    N, kw, mode, C1, C2 = c.n_cols, c.key_words, c.mode, c.cap, c.joint_cap
    cols = list(range(N)) if c.cols is None else [int(x) for x in c.cols]
    sums = [int(x) for x in fr.colsums_np(c.body, N, kw, mode)] if c.n_rows else [0] * N
    holders = [int(x) for x in pr.pan_expected_np(c.body, N, kw, mode)[1].sum(axis=0)] if c.n_rows else [0] * N
    for j, col in enumerate(cols):
        h = hist[j]
        assert sum(h[:C1 + 1]) == c.n_rows
        assert sum(b * h[b] for b in range(C1)) + h[C1 + 1] == sums[col]
        assert sum(h[1:C1 + 1]) == holders[col]
    full, _ = sr.spectra_expected_py(c.body, N, kw, mode, None, C2) if c.n_rows * N <= PY_ROAD_CELLS else (ints(sr.hist_expected_np(c.body, N, kw, mode, None, C2)), None)
    mins = dr.dist_expected_np(c.body, N, kw, mode, mins=True)[1] if mode == COUNT and c.n_rows else None
    pay = sr.split_payload(c.body, N, kw, mode) if c.n_rows else None
    for p, (x, y) in enumerate(c.pairs):
        J = joint[p]
        assert [sum(row) for row in J] == full[int(x)][:C2 + 1] and [sum(col) for col in zip(*J)] == full[int(y)][:C2 + 1]
        if x == y:
            assert all(J[a][b] == 0 for a in range(C2 + 1) for b in range(C2 + 1) if a != b)
        if mins is not None and int(max(pay[:, x].max(), pay[:, y].max())) < C2:
            assert sum(min(a, b) * J[a][b] for a in range(C2 + 1) for b in range(C2 + 1)) == int(mins[x][y])


def test_the_identities_where_no_count_reaches_the_cap():
    """a body of small counts, so that the identity with dist's sums of minima is not vacuous"""
    body = dr.make_body(5, 300, 9, 2, COUNT, fill=0.6, lo=1, hi=6)
    pairs = [(0, 1), (8, 3), (4, 4), (0, 1)]
    hist, joint = both(body, 9, 2, COUNT, None, 7, pairs, 7)
    mins = dr.dist_expected_np(body, 9, 2, COUNT, mins=True)[1]
    for p, (x, y) in enumerate(pairs):
        assert sum(min(a, b) * joint[p][a][b] for a in range(8) for b in range(8)) == int(mins[x][y]) > 0
    assert joint[0] == joint[3]
    assert all(h[7] == 0 and h[8] == 0 for h in hist)


def test_the_sweep_covers_what_it_says():
    cs = sr.gpu_cases()
    for mode in (COUNT, PA):
        mine = [c for c in cs if c.mode == mode]
        assert {c.n_cols for c in mine} >= set(sr.COLUMNS)
        assert {c.n_rows for c in mine} >= set(sr.ROWS)
        assert {c.key_words for c in mine} == {1, 2, 3, 4}
        assert {c.shape for c in mine} == set(sr.SHAPES) and {c.kind for c in mine} == set(sr.KINDS)
        assert {c.cap for c in mine} >= set(sr.CAPS1) and {c.joint_cap for c in mine} >= set(sr.CAPS2)
        assert {c.pair_kind for c in mine} >= set(sr.PAIR_KINDS)
        live = [c for c in mine if c.n_rows]
        # both sides of every switch, on bodies with rows: LDS bins or global atomics (HIST, COUNT), LDS tables or global atomics, gather or stream
        assert {c.cap <= sr.HIST_LDS_CAP for c in live} == {True, False}
        assert {(c.plan["lds"], c.plan["stream"]) for c in live} == {(a, b) for a in (True, False) for b in (True, False)}
        # several runs of rows a block and several blocks of columns, with LDS bins and without
        assert any(c.n_rows >= 4200 and c.n_cols > 64 and c.cap <= sr.HIST_LDS_CAP for c in mine) and any(c.n_rows >= 4200 and c.cap > sr.HIST_LDS_CAP for c in mine)
    assert sr.CAPS1 == [1, 2, 255, 254, 256, 65535] and sr.CAPS2 == [1, 2, 63, 108, 109, 110, 255]
    assert {len(c.pairs) for c in cs} >= {1, 2, 3, 4, 15, 16, 17, 70}
    assert any(len(c.pairs) >= 3 and any(x == y for x, y in c.pairs) and len({tuple(p) for p in c.pairs.tolist()}) < len(c.pairs) for c in cs)
    # the rule's two sides a byte apart, and a column apart
    rule = {c.name.rsplit("-", 1)[1]: c for c in cs if "-rule-j2-" in c.name and c.key_words == 1}
    assert (rule["rb512"].row_bytes, rule["rb512"].plan["stream"], rule["rb511"].row_bytes, rule["rb511"].plan["stream"]) == (512, False, 511, True)
    assert (rule["u2"].plan["U"], rule["u2"].plan["stream"], rule["u3"].plan["U"], rule["u3"].plan["stream"]) == (2, False, 3, True)
    # counts at C - 1, C, C + 1 and 2^32 - 1 reach both tables
    c = sr.case(next(c.name for c in cs if c.mode == COUNT and c.shape == "uniform" and c.n_rows == 4200 and c.cap == 254))
    vals = set(np.unique(sr.split_payload(c.body, c.n_cols, c.key_words, c.mode)).tolist())
    assert vals >= {c.cap - 1, c.cap, c.cap + 1, c.joint_cap - 1, c.joint_cap, c.joint_cap + 1, sr.U32}
    # the Python road walks every axis value but the widest matrices
    seen = [c for c in cs if walked(c)]
    assert {c.n_cols for c in seen} >= set(sr.COLUMNS) - {1025} and {c.n_rows for c in seen} >= set(sr.ROWS) and {c.cap for c in seen} >= set(sr.CAPS1)
    assert {c.joint_cap for c in seen} >= set(sr.CAPS2) and {c.shape for c in seen} == set(sr.SHAPES) and {c.mode for c in seen} == {COUNT, PA}
    # the constants the reference restates are the file's
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "spectra.hip")).read()
    for text in (f"SP_HIST_LDS_CAP = {sr.HIST_LDS_CAP};", f"SP_JOINT_LDS_CAP = {sr.JOINT_LDS_CAP};", f"SP_JOINT_LDS_WORDS = {sr.JOINT_LDS_WORDS};", f"SP_GROUP = {sr.GROUP};",
                 "SP_GATHER_FACTOR = 2;", "SP_BLOCK = 64;"):
        assert text in src, text


# ---- the statistics and the texts -------------------------------------------------------------------------------------------------------
def test_sample_statistics_by_hand():
    #        b: 0    1   2  3  4   5   6  7  (>= 8) volume
    h = [1000, 500, 90, 20, 30, 80, 80, 10, 3, 40]
    assert sr.sample_stats(h, 8) == dict(rows=813, singletons=500, volume=500 + 180 + 60 + 120 + 400 + 480 + 70 + 40, tail_volume=40, valley=3, peak=5)
    assert sr.sample_stats([5, 4, 3, 2, 1, 0], 4) == dict(rows=10, singletons=4, volume=4 + 6 + 6 + 0, tail_volume=0, valley=0, peak=1)      # no valley
    assert sr.sample_stats([5, 7, 7], 1) == dict(rows=7, singletons=7, volume=7, tail_volume=7, valley=0, peak=0)      # C1 = 1: no bin between
    assert sr.sample_stats([0, 1, 2, 9, 30], 2)["valley"] == 0 and sr.sample_stats([0, 1, 2, 9, 30], 2)["peak"] == 1      # b < C1 - 1 leaves no b at C1 = 2


def test_pair_statistics_by_hand():
    J = [[50, 4, 1], [6, 10, 0], [2, 0, 7]]      # a: x's count, b: y's
    s = sr.pair_stats(J, 2, solid=2, k=21)
    assert (s["both"], s["x_only"], s["y_only"]) == (17, 8, 5)
    assert s["jaccard"] == Fraction(17, 30) and s["completeness"] == Fraction(7, 9)
    assert abs(s["qv"] - (-10 * math.log10(1 - (1 - 5 / 22) ** (1 / 21)))) < 1e-9
    assert sr.pair_stats(J, 2, solid=1)["completeness"] == Fraction(17, 25) and sr.pair_stats(J, 2)["qv"] is None
    assert math.isinf(sr.pair_stats([[3, 0], [1, 2]], 1, k=31)["qv"]) and math.isnan(sr.pair_stats([[3, 0], [1, 0]], 1, k=31)["qv"])
    assert sr.pair_stats([[3, 4], [0, 0]], 1, k=31)["qv"] == 0.0 and sr.pair_stats([[3, 0], [0, 0]], 1)["jaccard"] is None


def tables(seed, M, cap, P, joint_cap, rows=5000):
    """tables of a random body, the pairs among its columns"""
    body = sr.spectra_body(seed, rows, M, 1, COUNT, "uniform" if seed % 2 else "skewed", (cap, joint_cap))
    pairs = sr.make_pairs("many", M, joint_cap, seed)[:P] if P else None
    return sr.spectra_expected_np(body, M, 1, COUNT, None, cap, pairs, joint_cap), pairs


@pytest.mark.parametrize("seed,M,cap,P,joint_cap,solid,k", [(1, 3, 255, 4, 63, 1, 31), (2, 5, 8, 6, 4, 3, 21), (3, 1, 1, 1, 1, 1, 127), (4, 9, 65535, 0, 0, 1, None),
                                                              (5, 4, 2, 5, 255, 255, 8), (6, 2, 300, 3, 2, 2, None)])
def test_from_tables_against_exact_fractions(seed, M, cap, P, joint_cap, solid, k, tmp_path):
    """the report printed from saved tables: integers exact, ratios within one unit of the last printed digit"""
    (hist, joint), pairs = tables(seed, M, cap, P, joint_cap)
    ids = [f"S{j}" for j in range(M)]
    id_pairs = [(ids[x], ids[y]) for x, y in pairs] if P else []
    (tmp_path / "h.tsv").write_text(sr.hist_text(ids, cap, hist))
    args = ["spectra", "--from-tables", tmp_path / "h.tsv"]
    if P:
        (tmp_path / "j.tsv").write_text(sr.joint_text(id_pairs, joint_cap, joint))
        args += ["--joint", tmp_path / "j.tsv", "--solid", solid] + (["--kmer-size", k] if k else [])
    r = kmx(*args)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    sr.check_report(r.stdout, ids, cap, hist, id_pairs, joint_cap, joint, solid, k)
    r2 = kmx(*args, "--output", tmp_path / "out.tsv")
    assert r2.returncode == 0 and r2.stdout == "" and open(tmp_path / "out.tsv").read() == r.stdout


def test_texts_are_pinned(tmp_path):
    hist = [[2, 1, 1, 3], [3, 0, 1, 3], [1, 0, 3, 10]]
    joint = [[[2, 0, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 0, 0], [0, 0, 3]]]
    ht = "# kmx spectra hist\n# samples: 3\n# cap: 2\n# id: A\n# id: B\n# id: C\nbin\t0\t1\t2\n0\t2\t3\t1\n1\t1\t0\t0\n2\t1\t1\t3\nvolume\t3\t3\t10\n"
    jt = "# kmx spectra joint\n# pairs: 2\n# cap: 2\n# pair: A\tB\n# pair: C\tC\npair\ta\tb\trows\n0\t0\t0\t2\n0\t1\t0\t1\n0\t2\t2\t1\n1\t0\t0\t1\n1\t2\t2\t3\n"
    assert sr.hist_text("ABC", 2, hist) == ht and sr.joint_text([("A", "B"), ("C", "C")], 2, joint) == jt
    (tmp_path / "h.tsv").write_text(ht); (tmp_path / "j.tsv").write_text(jt)
    r = kmx("spectra", "--from-tables", tmp_path / "h.tsv", "--joint", tmp_path / "j.tsv", "--kmer-size", 21)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ("# kmx spectra\n# samples: 3\n# cap: 2\n# pairs: 2\n# joint_cap: 2\n# solid: 1\n# kmer_size: 21\n" + sr.SAMPLE_COLUMNS + "\n"
                        "A\t2\t1\t4\t3\t0\t1\nB\t1\t0\t3\t3\t0\t1\nC\t3\t0\t10\t10\t0\t1\n" + sr.PAIR_COLUMNS + "\n"
                        "A\tB\t1\t1\t0\t0.500000\t0.500000\tinf\nC\tC\t3\t0\t0\t1.000000\t1.000000\tinf\n")
    r = kmx("spectra", "--from-tables", tmp_path / "h.tsv")
    assert r.returncode == 0 and r.stdout.startswith("# kmx spectra\n# samples: 3\n# cap: 2\n# pairs: 0\n# joint_cap: NA\n# solid: NA\n# kmer_size: NA\n") and sr.PAIR_COLUMNS not in r.stdout


def test_usage_is_pinned():
    r = kmx("spectra")
    assert r.returncode == 1 and r.stdout == "" and "usage: " + USAGE_RUN in r.stderr and "       " + USAGE_FROM in r.stderr
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert USAGE_RUN.replace(" | ", " \\| ") in readme and USAGE_FROM in readme


HT = "# kmx spectra hist\n# samples: 3\n# cap: 2\n# id: A\n# id: B\n# id: C\nbin\t0\t1\t2\n0\t2\t3\t1\n1\t1\t0\t0\n2\t1\t1\t3\nvolume\t3\t3\t10\n"
JT = "# kmx spectra joint\n# pairs: 2\n# cap: 2\n# pair: A\tB\n# pair: C\tC\npair\ta\tb\trows\n0\t0\t0\t2\n0\t1\t0\t1\n0\t2\t2\t1\n1\t0\t0\t1\n1\t2\t2\t3\n"


@pytest.mark.parametrize("which,edit,word", [
    ("h", lambda t: t.replace("# kmx spectra hist\n", ""), "# kmx spectra hist"),
    ("h", lambda t: t.replace("# samples: 3\n", ""), "samples and cap"),
    ("h", lambda t: t.replace("# cap: 2\n", ""), "samples and cap"),
    ("h", lambda t: t.replace("# cap: 2", "# cap: 0"), "cap outside"),
    ("h", lambda t: t.replace("# cap: 2", "# cap: 65536"), "cap outside"),
    ("h", lambda t: t.replace("# samples: 3", "# samples: 0"), "sample count"),
    ("h", lambda t: t.replace("# id: C\n", ""), "id lines"),
    ("h", lambda t: t.replace("bin\t0\t1\t2\n", "bin\t0\t1\n"), "column line"),
    ("h", lambda t: t.replace("1\t1\t0\t0\n", ""), "expected bin 1"),
    ("h", lambda t: t.replace("volume\t3\t3\t10\n", ""), "ends before"),
    ("h", lambda t: t.replace("volume\t3\t3\t10\n", "3\t3\t3\t10\n"), "volume line"),
    ("h", lambda t: t + "4\t0\t0\t0\n", "more than cap + 2"),
    ("h", lambda t: t.replace("1\t1\t0\t0\n", "1\t1\tx\t0\n"), "expected a number"),
    ("h", lambda t: t.replace("1\t1\t0\t0\n", "1\t-1\t0\t0\n"), "expected a number"),
    ("h", lambda t: t.replace("1\t1\t0\t0\n", "1\t1\t0\n"), "columns"),
    ("h", lambda t: t.replace("1\t1\t0\t0\n", "1\t2\t0\t0\n"), "do not count the same rows"),
    ("h", lambda t: t.replace("volume\t3\t3\t10\n", "volume\t3\t3\t5\n"), "volume of a last bin"),
    ("h", lambda t: t.replace("volume\t3\t3\t10\n", "volume\t0\t3\t10\n"), "volume of a last bin"),
    ("h", lambda t: "", "ends before"),
    ("j", lambda t: t.replace("# kmx spectra joint\n", ""), "# kmx spectra joint"),
    ("j", lambda t: t.replace("# pairs: 2\n", ""), "pairs and cap"),
    ("j", lambda t: t.replace("# cap: 2", "# cap: 256"), "cap outside"),
    ("j", lambda t: t.replace("# pair: C\tC\n", ""), "pair lines"),
    ("j", lambda t: t.replace("# pair: C\tC\n", "# pair: C\n"), "two sample ids"),
    ("j", lambda t: t.replace("pair\ta\tb\trows\n", "pair\ta\tb\n"), "column line"),
    ("j", lambda t: t.replace("0\t1\t0\t1\n", "0\t1\t0\n"), "four columns"),
    ("j", lambda t: t.replace("0\t1\t0\t1\n", "0\t3\t0\t1\n"), "outside the table"),
    ("j", lambda t: t.replace("1\t0\t0\t1\n", "2\t0\t0\t1\n"), "outside the table"),
    ("j", lambda t: t.replace("0\t1\t0\t1\n", "0\t1\t0\t0\n"), "no rows"),
    ("j", lambda t: t.replace("0\t0\t0\t2\n0\t1\t0\t1\n", "0\t1\t0\t1\n0\t0\t0\t2\n"), "order"),
    ("j", lambda t: t.replace("0\t1\t0\t1\n", "0\t1\t0\t1\n0\t1\t0\t1\n"), "order"),
    ("j", lambda t: t.replace("1\t2\t2\t3\n", "1\t2\t2\t4\n"), "does not count the rows"),
    ("j", lambda t: t.replace("0\t1\t0\t1\n", "0\t1\t0\tx\n"), "expected a number"),
    ("j", lambda t: "", "no table"),
])
def test_malformed_tables_are_refused(which, edit, word, tmp_path):
    (tmp_path / "h.tsv").write_text(edit(HT) if which == "h" else HT)
    (tmp_path / "j.tsv").write_text(edit(JT) if which == "j" else JT)
    r = kmx("spectra", "--from-tables", tmp_path / "h.tsv", "--joint", tmp_path / "j.tsv", "--output", tmp_path / "out")
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "" and word in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_from_tables_refuses_what_does_not_go_with_it(tmp_path):
    (tmp_path / "h.tsv").write_text(HT); (tmp_path / "j.tsv").write_text(JT)
    r = kmx("spectra", "--from-tables", tmp_path / "nothing.tsv")
    assert r.returncode == 1 and "nothing.tsv" in r.stderr and r.stdout == ""
    r = kmx("spectra", "--from-tables", tmp_path / "h.tsv", "--joint", tmp_path / "nothing.tsv")
    assert r.returncode == 1 and "nothing.tsv" in r.stderr and r.stdout == ""
    for extra in (("--samples", "x"), ("--gpus", 2), ("--cap", 2), ("--joint-cap", 2), ("--hist", "y"), ("--all-pairs",), ("--against", "A"), ("--pairs", "z"),
                  ("--run", "w"), ("--batch-mb", 1), ("--kmer-size", 31), ("--solid", 1), ("--joint", tmp_path / "j.tsv", "--solid", 3),
                  ("--joint", tmp_path / "j.tsv", "--solid", 0), ("--joint", tmp_path / "j.tsv", "--kmer-size", 7), ("--joint", tmp_path / "j.tsv", "--kmer-size", 128)):
        r = kmx("spectra", "--from-tables", tmp_path / "h.tsv", *extra)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", extra


# ---- header, binding, sources -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_spectra_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"SPECTRA_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no SPECTRA_EXPORTS"
    bound = set(re.findall(r'"(kmx_spectra_\w+)"', listed.group(1)))
    want = {"kmx_spectra_dev", "kmx_spectra_host"} | {"kmx_spectra_result_" + s for s in ("wait", "hist_dev", "joint_dev", "copy_hist", "copy_joint", "kernel_ms",
                                                                                        "kernel_parts_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert "kmx_spectra_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]      # the opening list of entry points
    assert "/* ---------------------------------------------------------------- spectra */" in hdr
    assert hdr.index("/* ------------------------------------------------------------------ match */") < hdr.index("- spectra */") < hdr.index("- count */")
    assert re.search(r"#define KMX_SPECTRA_HIST  1u\b", hdr) and re.search(r"#define KMX_SPECTRA_JOINT 2u\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_spectra_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == ["key_words", "mode", "n_cols", "n_use", "rows", "n_rows", "cols", "pairs", "n_pairs", "cap1", "cap2", "flags", "hist", "joint"]
    struct_src = re.search(r"class KmxSpectraTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    for name in ("KmxSpectraTask", "SpectraResult", "SpectraOutput", "def spectra(", "def spectra_dev("):
        assert name in src, name
    host = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "matrix_host.hpp")).read()
    assert "kmx_spectra_*" in host and "spectra.hip" in host


def test_library_and_binding_structures():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert so.kmx_version() == 2
    assert len(lib.SPECTRA_EXPORTS) == 11
    for name in lib.SPECTRA_EXPORTS:
        assert hasattr(so, name), name
    T = lib.KmxSpectraTask
    assert ctypes.sizeof(T) == 80 and T.cols.offset == 32 and T.pairs.offset == 40 and T.n_pairs.offset == 48 and T.flags.offset == 60 and T.hist.offset == 64 and T.joint.offset == 72
    assert (lib.SPECTRA_HIST, lib.SPECTRA_JOINT) == (1, 2)
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "spectra.hip")).read()
    assert "static_assert(sizeof(kmx_spectra_task) == 80" in src


def test_spectra_hip_has_knobs_of_its_own_and_plain_atomics():
    csrc = os.path.join(ROOT, "kmtricks_amd", "csrc")
    src = open(os.path.join(csrc, "spectra.hip")).read()
    for word in ("kmx_plan_cus", "kmx_grid_cap", "KMX_PLAN_CUS", "KMX_MAX_GRID", "KMX_PAN_", "asm"):
        assert word not in src, word
    assert 'kmx_env_cus("KMX_SPECTRA_CUS", ctx)' in src and 'kmx_env_grid("KMX_SPECTRA_GRID", dflt)' in src
    assert "spectra.hip" in open(os.path.join(csrc, "Makefile")).read()
    mk = open(os.path.join(ROOT, "kmtricks_amd", "host", "Makefile")).read()
    assert "kmx_spectra.cpp" in mk and "kmx_spectra_stats.hpp" in mk
    stats = open(os.path.join(ROOT, "kmtricks_amd", "host", "kmx_spectra_stats.hpp")).read()
    assert "hip" not in stats.lower()


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output, nothing written ---------------
MODES = ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxspectra")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in MODES:
        rmode = dr.KINDS[mode][5]
        bodies = [dr.make_body(p, 10, 3, 1, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    return dict(dir=d, runs=out, ids=ids, k=k)


def refused(tmp_path, *args, word=None, pairs=True):
    outs = [tmp_path / n for n in ("out.tsv", "hist.tsv", "joint.tsv")]
    r = kmx("spectra", *args, "--output", outs[0], "--hist", outs[1], *(("--joint", outs[2]) if pairs else ()))
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert word is None or word in r.stderr, (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert not any(os.path.exists(p) for p in outs), "a refusal wrote a file"


def text_file(tmp_path, text, name="s.txt"):
    with open(tmp_path / name, "w") as f:
        f.write(text)
    return tmp_path / name


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_bad_options(runs, tmp_path, mode):
    run = runs["runs"][mode]
    refused(tmp_path, "--run", tmp_path / "nothing", "--all-pairs", word="not a kmtricks runtime directory")
    refused(tmp_path, "--run", run, "--all-pairs", "--frobnicate")
    for v in (0, 65536, "-1", "many"):
        refused(tmp_path, "--run", run, "--all-pairs", "--cap", v, word="--cap")
    for v in (0, 256, "-1"):
        refused(tmp_path, "--run", run, "--all-pairs", "--joint-cap", v, word="--joint-cap")
    refused(tmp_path, "--run", run, "--all-pairs", "--solid", 0, word="--solid")
    refused(tmp_path, "--run", run, "--all-pairs", "--solid", 64, word="--solid")
    refused(tmp_path, "--run", run, "--all-pairs", "--joint-cap", 3, "--solid", 4, word="--solid")
    for g in (0, 17, "two"):
        refused(tmp_path, "--run", run, "--all-pairs", "--gpus", g, word="--gpus")
    refused(tmp_path, "--run", run, "--all-pairs", "--batch-mb", "lots", word="--batch-mb")
    refused(tmp_path, "--run", run, "--all-pairs", "--samples")
    refused(tmp_path, "--run", run, "--all-pairs", "--kmer-size", 31, word="--kmer-size")
    refused(tmp_path, "--run", run, "--all-pairs", "--against", "A", word="exclude each other")
    refused(tmp_path, "--run", run, "--pairs", text_file(tmp_path, "A B\n", "p.txt"), "--against", "A", word="exclude each other")
    refused(tmp_path, "--run", run, word="need pairs")                                     # --joint without pairs
    refused(tmp_path, "--run", run, "--joint-cap", 3, word="need pairs", pairs=False)
    refused(tmp_path, "--run", run, "--solid", 1, word="need pairs", pairs=False)
    refused(tmp_path, "--run", run, "--against", "D", word="D is not in the run")
    refused(tmp_path, "--run", run, "--against", "A", "--samples", text_file(tmp_path, "A\n"), word="no other sample")
    refused(tmp_path, "--run", run, "--all-pairs", "--samples", text_file(tmp_path, "B\n"), word="two listed samples")


@pytest.mark.parametrize("text,word", [
    ("A D\n", "D is not in the run"),            # an id that is not in the fof
    ("A\n", "expected two sample ids"),
    ("A B C\n", "expected two sample ids"),
    ("", "names no pair"),
    ("\n \n", "names no pair"),
])
def test_driver_refuses_bad_pair_lists(runs, tmp_path, text, word):
    for mode in ("kmer:count:bin", "hash:pa:bin"):
        refused(tmp_path, "--run", runs["runs"][mode], "--pairs", text_file(tmp_path, text, "p.txt"), word=word)
    refused(tmp_path, "--run", runs["runs"]["kmer:pa:bin"], "--pairs", tmp_path / "nothing.txt", word="nothing.txt")
    refused(tmp_path, "--run", runs["runs"]["kmer:pa:bin"], "--all-pairs", "--samples", text_file(tmp_path, "A\nB\nA\n"), word="A is named twice")


def test_driver_refuses_tables_past_the_limit(runs, tmp_path):
    """--all-pairs names the 8 GiB limit: 400 samples are 79 800 pairs of 65 536 cells"""
    ids = [f"S{j}" for j in range(400)]
    body = dr.make_body(3, 4, 400, 1, PA)
    root = dr.write_run(runs["dir"] / "wide", "hash:pa:bin", 31, ids, [body], window=16)
    refused(tmp_path, "--run", root, "--all-pairs", "--joint-cap", 255, word="8 GiB")
    refused(tmp_path, "--run", root, "--all-pairs", "--joint-cap", 255, word="--all-pairs")


def test_driver_refuses_modes_it_does_not_read(runs, tmp_path):
    body = dr.make_body(1, 4, 3, 1, COUNT)
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused(tmp_path, "--run", root, "--all-pairs", word=said)
