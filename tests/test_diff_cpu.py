"""CPU-only: tests/diff_ref.py (the judge of `kmx diff`) against the examples the header works by hand, its two roads against each
other, the threshold, the condition under which the GPU test may compare keep sets (no row of its inputs inside the tolerance band of
its threshold), the new symbols of the C ABI as the header and the binding name them, and the refusals of `kmx diff` that come before
any device is asked for, on run directories written by hand."""
import ctypes
import math
import os
import re
import shutil
import struct
import subprocess
import numpy as np
import pytest

import dist_ref as dr
import diff_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = fr.MODE_COUNT, fr.MODE_PA
CHI2_05 = 3.841458820694126


def both(body, N, kw, mode, group, T0, T1):
    """the two roads: integers equal, the float64 statistic within the derived tolerance of the mpmath one -> (py rows, np records)"""
    py, nq = fr.diff_expected_py(body, N, kw, mode, [int(g) for g in group], T0, T1), fr.diff_expected_np(body, N, kw, mode, group, T0, T1)
    assert len(py) == len(nq)
    for r, (a, b) in enumerate(zip(py, nq)):
        assert (a["c0"], a["c1"], a["r0"], a["r1"], a["over"], r) == (int(b["sum_ctrl"]), int(b["sum_case"]), int(b["rec_ctrl"]), int(b["rec_case"]), int(b["over"]), int(b["row"]))
        assert abs(a["stat"] - float(b["stat"])) <= a["tol"], (r, a, b)
    return py, nq


def test_worked_examples():
    """the examples of include/kmx.h, section diff, as literals, and their group swap"""
    key = bytes(8)
    rows = ((0, 0, 5, 5), (3, 3, 3, 3), (1, 2, 4, 8))
    cnt = b"".join(key + struct.pack("<4I", *row) for row in rows)
    py, nq = both(cnt, 4, 1, COUNT, (0, 0, 1, 1), 100, 100)
    assert [(x["c0"], x["c1"], x["over"]) for x in py] == [(0, 10, 1), (6, 6, 0), (3, 12, 1)]
    assert float(nq["stat"][0]) == 13.862943611198906 == 20 * math.log(2)
    assert float(nq["stat"][1]) == 0.0 and py[1]["stat"] == 0
    assert abs(float(nq["stat"][2]) - 5.7823427) < 1e-7 and abs(float(py[2]["stat"]) - 5.7823427) < 1e-7
    assert [(x["r0"], x["r1"]) for x in py] == [(0, 2), (2, 2), (2, 2)]
    kept, band = fr.keep_expected(py, CHI2_05)
    assert kept == [True, False, True] and not any(band)
    sw, nsw = both(cnt, 4, 1, COUNT, (1, 1, 0, 0), 100, 100)
    assert [x["over"] for x in sw] == [2, 0, 2]
    assert [float(x) for x in nsw["stat"]] == [float(x) for x in nq["stat"]]
    # presence/absence rows: a sample's count is its bit; every padding bit set
    pa = b"".join(key + bytes([b | 0xF0]) for b in (0b1100, 0b1111, 0b0100))
    py, _ = both(pa, 4, 1, PA, (0, 0, 1, 1), 100, 100)
    assert [(x["c0"], x["c1"], x["r0"], x["r1"], x["over"]) for x in py] == [(0, 2, 0, 2, 1), (2, 2, 2, 2, 0), (0, 1, 0, 1, 1)]
    # an ignored column changes nothing
    cnt5 = b"".join(key + struct.pack("<5I", *(row[:2] + (999,) + row[2:])) for row in rows)
    py5, _ = both(cnt5, 5, 1, COUNT, (0, 0, 2, 1, 1), 100, 100)
    assert [(x["c0"], x["c1"], x["r0"], x["r1"]) for x in py5] == [(0, 10, 0, 2), (6, 6, 2, 2), (3, 12, 2, 2)]
    assert fr.DIFF_REC.itemsize == 40


def test_the_two_roads_agree():
    """N 2 ... 130 with every padding bit set; fills 0, 0.02, 0.5 and 1; counts including 2^32 - 1"""
    fills = (0.0, 0.02, 0.5, 1.0)
    for N in range(2, 131):
        fill, kw = fills[N % 4], 1 + N % 4
        rows = 1 + (N * 7) % 23
        g = fr.random_groups(N, N) if N > 2 else np.array([0, 1], np.uint8)
        for mode in (PA, COUNT):
            body = fr.make_body(N + 1000 * mode, rows, N, kw, mode, fill, maxed=0.3, group=g, effect=0.2)
            py_s, np_s = fr.colsums_py(body, N, kw, mode), fr.colsums_np(body, N, kw, mode)
            assert py_s == [int(x) for x in np_s]
            T0, T1 = fr.totals_of(np_s, g)
            py, _ = both(body, N, kw, mode, g, T0 or 7, T1 or 5)
            if fill == 1.0 and mode == PA:      # a padding bit that reached a result would show here
                assert all(x["c0"] == int((g == 0).sum()) and x["c1"] == int((g == 1).sum()) for x in py if x["r0"])
    # counts of 2^32 - 1 in every column: sums pass 2^32
    body = fr.make_body(1, 5, 9, 1, COUNT, 1.0, lo=0xFFFFFFFF, hi=0x100000000)
    py, _ = both(body, 9, 1, COUNT, [0, 1, 0, 1, 0, 1, 0, 1, 2], 2 ** 40, 2 ** 41 + 1)
    assert all(x["c0"] == x["c1"] == 4 * 0xFFFFFFFF for x in py) and fr.colsums_py(body, 9, 1, COUNT) == [5 * 0xFFFFFFFF] * 9


def test_statistic_tolerance_over_wide_operands():
    """the float64 road against mpmath within the derived tolerance, counts up to 2^41 and totals up to 2^49"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(2000):
        c0, c1 = (int(rng.integers(0, 2 ** int(rng.integers(1, 42)))) for _ in range(2))
        T0, T1 = (int(rng.integers(1, 2 ** int(rng.integers(1, 50)))) for _ in range(2))
        s, tol = fr.stat_mp(c0, c1, T0, T1)
        got = float(fr.stat_np([c0], [c1], T0, T1)[0])
        assert abs(s - got) <= tol, (c0, c1, T0, T1, got, float(s))
        if tol:
            worst = max(worst, float(abs(s - got) / tol) * 16)
    assert worst < 16


def test_threshold():
    assert abs(fr.threshold(0.05) / CHI2_05 - 1) <= 1e-12
    assert abs(fr.threshold(5e-11) / 43.17719790924114 - 1) <= 1e-12
    for p in (0.05, 5e-11, 0.5, 1e-3, 1e-300):
        t = fr.threshold(p)
        assert fr.pvalue(t) <= p < fr.pvalue(math.nextafter(t, 0.0)), p
    assert fr.threshold(1.0) == 0.0
    for p in (-1e-9, math.nan):      # (a statistic of 2000 has p = 0 in double: only these lie below it)
        with pytest.raises(ValueError):
            fr.threshold(p)


def test_no_row_of_the_gpu_inputs_lies_in_the_band():
    """what lets tests/test_diff_gpu.py compare keep sets exactly: for every body / threshold pair it uses, no row's statistic is
    within its tolerance of the threshold.  The kept shares the GPU test promises are here too."""
    cases = fr.gpu_cases()
    assert len({c.name for c in cases}) == len(cases) >= 80
    for c in cases:
        assert len(c.rows) == c.n_rows and set(np.unique(c.group)) <= {0, 1, 2} and (c.group == 0).any() and (c.group == 1).any()
        assert c.totals[0] > 0 and c.totals[1] > 0
        for thr in c.thresholds:
            kept, band = fr.keep_expected(c.rows, thr, c.min_rec)
            assert not any(band), (c.name, thr, [i for i, b in enumerate(band) if b])
    for m in ("count", "pa"):
        c = fr.case(f"shares-{m}")
        shares = [sum(fr.keep_expected(c.rows, t)[0]) / c.n_rows for t in c.thresholds]
        assert 0.0005 <= shares[0] <= 0.003 and 0.45 <= shares[1] <= 0.6 and shares[2] == 1.0, shares
        z = fr.case(f"zeros-{m}")
        assert all(x["stat"] == 0 for x in z.rows)
        assert all(x["r0"] == x["r1"] == 0 and x["c0"] == x["c1"] == 0 for x in fr.case(f"ignored-{m}").rows)
    big = fr.case("ones-count-own")
    assert big.rows[0]["c0"] == int((big.group == 0).sum()) * 0xFFFFFFFF > 2 ** 40
    # the cases at the end of the list: count columns beyond the 1024 whose groups a lane keeps in a register, ignored ones among
    # them and columns that count; the long rows of the chunk sweep, whose p = 0.05 keep sets are proper subsets
    for N, _ in fr.WIDE_COUNT_COLS:
        c = fr.case(f"cols-count-{N}")
        assert N > 1024 and c.group[1024] == fr.IGN and c.thresholds[0] == 0.0 and math.isinf(c.thresholds[2])
        pay = dr.split_payload(c.body, N, 1, COUNT)
        assert pay[:, 1024:].any(axis=1).sum() >= 20      # rows that hold a count out there: a group read wrong shows in their sums
    assert set(fr.case("cols-count-1100").group[1025:].tolist()) == {0, 1, 2}
    for m, N in (("count", 70), ("pa", 520)):
        for rows in fr.RW_ROWS:
            c = fr.case(f"rw-{m}-{rows}")
            n = sum(fr.keep_expected(c.rows, c.thresholds[1])[0])
            assert c.n_cols == N and c.n_rows == rows and 0 < n < rows, (c.name, n)
        assert {fr.case(f"rw-{m}-{rows}").key_words for rows in fr.RW_ROWS} == {1, 2, 3, 4}


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_(?:diff|colsums)_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"DIFF_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no DIFF_EXPORTS"
    bound = set(re.findall(r'"(kmx_(?:diff|colsums)_\w+)"', listed.group(1)))
    want = ({"kmx_colsums_dev", "kmx_colsums_host"} | {"kmx_colsums_result_" + s for s in ("wait", "sums_dev", "copy_sums", "kernel_ms", "algo_bytes", "free")} |
            {"kmx_diff_dev", "kmx_diff_host"} | {"kmx_diff_result_" + s for s in ("wait", "rows", "row_bytes", "body_bytes", "body_dev", "copy_body", "recs_dev",
                                                                                  "copy_recs", "kernel_ms", "algo_bytes", "free")})
    assert declared == want == bound
    assert "kmx_diff_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]      # the opening list of entry points
    assert "/* ------------------------------------------------------------------- diff */" in hdr
    # the binding's structures have the header's fields in the header's order
    for cname, pyname in (("kmx_colsums_task", "KmxColsumsTask"), ("kmx_diff_task", "KmxDiffTask")):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr, re.S).group(1), flags=re.S)
        c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
        struct_src = re.search(r"class %s\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n" % pyname, src, re.S).group(1)
        assert c_fields == re.findall(r'\("(\w+)"', struct_src), cname
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_diff_rec;", hdr, re.S).group(1), flags=re.S)
    assert [d.split()[-1] for d in body.split(";") if d.strip()] == list(fr.DIFF_REC.names)
    for name in ("KmxColsumsTask", "KmxDiffTask", "DiffResult", "DiffOutput", "def diff(", "def diff_dev(", "def colsums(", "def colsums_dev("):
        assert name in src, name


def test_library_and_binding_structures():
    """the built library has the symbols (kmx_version unchanged); the binding's structures have the C sizes; a record is 40 bytes"""
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert so.kmx_version() == 2
    assert len(lib.DIFF_EXPORTS) == 21
    for name in lib.DIFF_EXPORTS:
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxColsumsTask) == 40 and ctypes.sizeof(lib.KmxDiffTask) == 64
    assert lib.DIFF_REC.itemsize == 40 and lib.DIFF_REC == fr.DIFF_REC
    assert lib.KmxDiffTask.threshold.offset == 56 and lib.KmxDiffTask.group.offset == 32


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output -------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def refused(*args, word=None):
    r = kmx("diff", *args)
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert word is None or word in r.stderr, (args, r.stderr)


MODES = ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxdiff")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in MODES:
        rmode = dr.KINDS[mode][5]
        bodies = [fr.make_body(p, 10, 3, 1, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    with open(d / "groups.txt", "w") as f:
        f.write("A control\nB\tcase\n")
    return dict(dir=d, runs=out, ids=ids, k=k, groups=d / "groups.txt")


def test_driver_refuses_bad_options(runs, tmp_path):
    run, groups = runs["runs"]["kmer:count:bin"], runs["groups"]
    refused(word="--run")
    refused("--run", run, word="--groups")
    refused("--run", tmp_path / "nothing", "--groups", groups, word="not a kmtricks runtime directory")
    refused("--run", run, "--groups", tmp_path / "nothing.txt", word="nothing.txt")
    refused("--run", run, "--groups", groups, "--frobnicate")
    refused("--run", run, "--groups", groups, "--correction", "bh", word="--correction")
    for a in ("0", "1", "-0.1", "1.5", "nan", "five"):
        refused("--run", run, "--groups", groups, "--alpha", a, word="--alpha")
    for g in (0, 17, "two"):
        refused("--run", run, "--groups", groups, "--gpus", g, word="--gpus")
    refused("--run", run, "--groups", groups, "--min-rec", "-1", word="--min-rec")


@pytest.mark.parametrize("text,word", [
    ("A control\nB case\nD case\n", "D is not in the run"),           # an id that is not in the fof
    ("A control\nB case\nA case\n", "A is named twice"),               # a duplicate
    ("A control\nB cases\n", "neither case nor control"),              # another label
    ("A control\nB\n", "expected"),                                    # no label
    ("A control\nB case extra\n", "expected"),                         # a third word
    ("A control\nC control\n", "no case sample"),                      # an empty group
    ("B case\n", "no control sample"),
    ("", "no control sample"),
])
def test_driver_refuses_bad_groups_files(runs, tmp_path, text, word):
    with open(tmp_path / "g.txt", "w") as f:
        f.write(text)
    for mode in ("kmer:count:bin", "hash:pa:bin"):
        refused("--run", runs["runs"][mode], "--groups", tmp_path / "g.txt", word=word)


def test_driver_refuses_modes_it_does_not_read(runs):
    body = fr.make_body(1, 4, 3, 1, COUNT)
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text", "kmer:pa:text", "hash:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused("--run", root, "--groups", runs["groups"], word=said)


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_files_that_do_not_fit(runs, mode, tmp_path):
    ext, hdr, magic, cols_at, kw, rmode = dr.KINDS[mode]
    src = runs["runs"][mode]
    f1 = os.path.join("matrices", f"matrix_1.{ext}")

    def variant(name):
        shutil.copytree(src, tmp_path / name)
        return tmp_path / name

    d = variant("cut")           # a truncated body: no whole number of rows
    with open(d / f1, "r+b") as f:
        f.truncate(os.path.getsize(d / f1) - 1)
    refused("--run", d, "--groups", runs["groups"], word=f"matrix_1.{ext}")
    d = variant("gone")          # a missing matrix
    os.remove(d / f1)
    refused("--run", d, "--groups", runs["groups"], word=f"matrix_1.{ext}")
    d = variant("cols")          # a header of another number of columns than the fof has samples
    with open(d / f1, "r+b") as f:
        f.seek(cols_at); f.write(struct.pack("<I", 4))
    refused("--run", d, "--groups", runs["groups"], word=f"matrix_1.{ext}")
    d = variant("magic")         # another kind of file under the name
    with open(d / f1, "r+b") as f:
        f.seek(13); f.write(struct.pack("<Q", 0x1234))
    refused("--run", d, "--groups", runs["groups"], word="Invalid file format")
