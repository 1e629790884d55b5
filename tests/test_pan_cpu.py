"""CPU-only: tests/pan_ref.py (the judge of `kmx pan`) against the example the header works by hand, its two roads against each other, the
five identities, the closed-form curves against brute force over every order of adding the samples, `kmx pan --from-spectrum` against
exact fractions, the texts of the driver, the new symbols of the C ABI as the header and the binding name them, and the refusals of
`kmx pan` that come before any device is asked for, on run directories written by hand."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dist_ref as dr
import pan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = pr.MODE_COUNT, pr.MODE_PA
USAGE_RUN = ("kmx pan --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
             "[--min-abund INT] [--shared FILE] [--spectrum FILE] [--output FILE] [--gpus INT] [--batch-mb INT] [-v]")
USAGE_FROM = "kmx pan --from-spectrum FILE [--output FILE]"


def both(body, N, kw, mode, cols=None, a=1):
    """the two roads, equal -> (spectrum, shared) as lists of lists of integers"""
    s1, h1 = pr.pan_expected_py(body, N, kw, mode, cols, a)
    s2, h2 = pr.pan_expected_np(body, N, kw, mode, cols, a)
    assert s1 == [[int(x) for x in row] for row in s2] and h1 == [[int(x) for x in row] for row in h2], (N, kw, mode, cols, a)
    return s1, h1


def count_rows(rows, kw=1):
    return b"".join(bytes(range(1, 8 * kw + 1)) + struct.pack(f"<{len(r)}I", *r) for r in rows)


def test_worked_example():
    """the example of include/kmx.h, section pan, as literals"""
    body = count_rows([(1, 0, 2, 0), (0, 0, 0, 5), (3, 3, 3, 3), (0, 0, 0, 0)])
    spec, shared = both(body, 4, 1, COUNT)
    assert spec == [[1, 1, 1, 0, 1], [2, 0, 0, 1, 1], [2, 1, 0, 0, 1]]
    assert shared == [[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]]
    # a = 3: the first row has rec 0
    spec, shared = both(body, 4, 1, COUNT, a=3)
    assert spec[0] == [2, 1, 0, 0, 1] and shared[2] == [0, 0, 0, 0] and shared[1] == [0, 0, 0, 1]
    # cols = (3, 0): the second row has rec 1, first 0, gap 1
    spec, shared = both(count_rows([(0, 0, 0, 5)]), 4, 1, COUNT, cols=(3, 0))
    assert spec == [[0, 1, 0], [1, 0, 0], [0, 1, 0]] and shared == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]
    spec, shared = both(body, 4, 1, COUNT, cols=(3, 0))
    assert spec == [[1, 2, 1], [2, 1, 1], [2, 1, 1]] and shared == [[0, 0, 0, 0], [1, 0, 0, 1], [1, 0, 0, 1]]
    # the same rows as presence/absence bits, every padding bit set
    pa = b"".join(bytes(8) + bytes([b | 0xF0]) for b in (0b0101, 0b1000, 0b1111, 0b0000))
    assert both(pa, 4, 1, PA) == both(body, 4, 1, COUNT)


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_the_two_roads_agree_and_the_identities_hold(mode):
    """N 1 ... 130, every padding bit set, fills 0 / 0.02 / 0.5 / 1, counts of 2^32 - 1, lists of every kind; the five identities"""
    for N in range(1, 131):
        fill = (0.0, 0.02, 0.5, 1.0)[N % 4]
        kw = 1 + N % 4
        rows = 1 + (N * 7) % 23
        body = pr.make_body(400 + N, rows, N, kw, mode, fill=fill, pad_ones=True, maxed=0.2, lo=1, hi=4)
        if mode == PA and N % 8:
            assert (np.asarray(body).reshape(rows, -1)[:, -1] >> (N % 8)).min() == 0xFF >> (N % 8)
        kind = pr.KINDS[N % len(pr.KINDS)]
        cols = pr.make_cols(kind, N, N)
        for a in ((1, 2, pr.U32)[N % 3], 1) if mode == COUNT else (1,):
            spec, shared = both(body, N, kw, mode, cols, a)
            pay = dr.split_payload(body, N, kw, mode)
            holders = (pay >= a).sum(axis=0) if mode == COUNT else pay.sum(axis=0)
            pr.check_identities(spec, shared, rows, cols, N, holders)
            if a == 1 and N <= 40:      # the presence tally of `kmx dist`: inter[c][c]
                inter = dr.dist_expected_np(body, N, kw, mode)[0]
                listed = np.zeros(N, bool); listed[np.arange(N) if cols is None else cols] = True
                assert [int(x) for x in np.asarray(shared).sum(axis=0)] == [int(inter[c][c]) if listed[c] else 0 for c in range(N)]


def test_the_sweep_covers_what_it_says():
    """every value of the issue's table appears in the list tests/test_pan_gpu.py walks, in both modes"""
    cases = pr.gpu_cases()
    for mode in (COUNT, PA):
        mine = [c for c in cases if c.mode == mode]
        assert {c.n_cols for c in mine} >= set(pr.COLUMNS) | {pr.LDS_MAX_M, pr.LDS_MAX_M + 1}
        assert {c.n_use for c in mine} >= {pr.LDS_MAX_M, pr.LDS_MAX_M + 1}      # both sides of the end of the LDS histograms
        assert {c.n_rows for c in mine} >= set(pr.ROWS)
        assert {c.key_words for c in mine} == {1, 2, 3, 4}
        assert {c.name.split("-")[2] for c in mine} >= set(pr.KINDS)
        assert {c.name.split("-")[5] for c in mine} >= {str(s) for s in pr.SHAPES}
        assert any(c.n_cols > pr.LDS_MAX_M and c.n_use <= pr.LDS_MAX_M for c in mine)      # a list that leaves far columns
    assert {a for c in cases for a in c.abunds} == {1, 2, pr.U32}
    # the shapes are what they say
    c = pr.case("c-9-none-r12293-k1-same-long")
    assert list(np.flatnonzero(c.expected[1][0][0])) == [4]
    c = pr.case("p-65-reversed-r12293-k1-uniform-long")
    assert (c.expected[1][0][0] > 0).all()
    c = pr.case("c-130-scattered-r4200-k1-skewed-long")
    assert len(np.flatnonzero(c.expected[1][0][0])) <= 3


# ---- the curves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,rows,fill", [(1, 5, 0.5), (2, 9, 0.5), (3, 12, 0.4), (4, 20, 0.6), (5, 25, 0.3), (6, 30, 0.5), (6, 8, 1.0), (5, 7, 0.0)])
def test_closed_forms_equal_the_average_over_all_orders(M, rows, fill):
    """pan_mean / core_mean / new_mean from the spectrum equal the average over ALL M! orders computed on the matrix itself, as exact
    Fractions; pan_order / core_order equal brute force in list order, for several lists"""
    N = M + 2
    body = pr.make_body(70 + M, rows, N, 1, PA, fill=fill)
    for cols in (np.arange(M), np.arange(N)[::-1][:M], np.random.default_rng(M).permutation(N)[:M]):
        spec, _ = pr.pan_expected_py(body, N, 1, PA, cols)
        exact = pr.curves_exact(spec)
        present = dr.split_payload(body, N, 1, PA)[:, cols]
        mean, pan_o, core_o = pr.curves_brute(present)
        assert exact["pan_mean"] == mean["pan"] and exact["core_mean"] == mean["core"] and exact["new_mean"] == mean["new"]
        assert exact["pan_order"] == pan_o and exact["core_order"] == core_o
        for m in range(2, M + 1):
            assert exact["new_mean"][m] == exact["pan_mean"][m] - exact["pan_mean"][m - 1]
        assert exact["new_mean"][1] == exact["pan_mean"][1]


def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def spectrum_of(h):
    """a spectrum with rows-by-recurrence h: every row holds the first rec samples of the list"""
    M = len(h) - 1
    first = [sum(h[1:])] + [0] * (M - 1) + [h[0]] if M >= 1 else [h[0]]
    return [list(h), first, list(h)]


def spectra():
    rng = np.random.default_rng(11)
    out = {"m1": [3, 7], "m2": [0, 5, 9], "m5": [2, 100, 30, 0, 7, 50]}
    out["m5-private"] = [0, 1000, 0, 0, 0, 0]
    out["m64"] = [int(x) for x in rng.integers(0, 10 ** 6, 65)]
    out["m64-core"] = [0] * 64 + [12345]
    h = [0] * 1001
    for r in list(rng.integers(1, 1001, 40)) + [1, 2, 1000]:
        h[int(r)] = int(rng.integers(1, 10 ** 5))
    out["m1000"] = h
    big = [0] * 1001
    big[1], big[2], big[500], big[1000] = 6 * 10 ** 9, 10 ** 9, 2 * 10 ** 9, 10 ** 9 + 7      # the sum about 10^10
    out["m1000-big"] = big
    out["m1000-private"] = [5] + [10 ** 7] + [0] * 999
    return out


@pytest.mark.parametrize("name", list(spectra()))
def test_from_spectrum_against_exact_fractions(name, tmp_path):
    """|value - exact| <= 10^-9 * sum(h) + 5 * 10^-7 (the roundings of the ratio recurrences, and %.6f); the
    ordered curves exactly; heaps_alpha to 10^-6 against Python's evaluation of the exact new_mean"""
    h = spectra()[name]
    M = len(h) - 1
    spec = spectrum_of(h)
    ids = [f"S{j}" for j in range(M)]
    path = tmp_path / "spec.tsv"
    path.write_text(pr.spectrum_text(ids, 3, spec))
    r = kmx("pan", "--from-spectrum", path)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    head, rows = pr.parse_curves(r.stdout)
    assert head["samples"] == str(M) and head["rows"] == str(sum(h)) and head["min_abund"] == "3"
    exact = pr.curves_exact(spec)
    tol = Fraction(sum(h), 10 ** 9) + Fraction(5, 10 ** 7)
    worst = Fraction(0)
    for m, sid, pan, core, new, pan_o, core_o in rows:
        assert sid == ids[m - 1] and pan_o == exact["pan_order"][m] and core_o == exact["core_order"][m]
        for got, key in ((pan, "pan_mean"), (core, "core_mean"), (new, "new_mean")):
            err = abs(Fraction(got) - exact[key][m])
            worst = max(worst, err)
            assert err <= tol, (name, m, key, got, float(exact[key][m]))
    print(f"{name}: worst error {float(worst):.3e}, allowed {float(tol):.3e}")
    alpha = pr.heaps_alpha(exact["new_mean"])
    assert not head["heaps_alpha"].startswith("-0.000000")
    if alpha is None:
        assert head["heaps_alpha"] == "NA"
    else:
        assert M >= 5 and abs(float(head["heaps_alpha"]) - alpha) <= 1e-6, (head["heaps_alpha"], alpha)
    # --output writes the same text and prints nothing
    r2 = kmx("pan", "--from-spectrum", path, "--output", tmp_path / "curves.tsv")
    assert r2.returncode == 0 and r2.stdout == "" and open(tmp_path / "curves.tsv").read() == r.stdout


def test_heaps_alpha_cases():
    s = spectra()
    assert pr.heaps_alpha(pr.curves_exact(spectrum_of(s["m1"]))["new_mean"]) is None      # fewer than 3 points
    assert pr.heaps_alpha(pr.curves_exact(spectrum_of(s["m2"]))["new_mean"]) is None
    assert pr.heaps_alpha(pr.curves_exact(spectrum_of(s["m64-core"]))["new_mean"]) is None      # nothing new after the first sample
    assert abs(pr.heaps_alpha(pr.curves_exact(spectrum_of(s["m5-private"]))["new_mean"])) < 1e-12      # every sample brings as much
    assert pr.heaps_alpha(pr.curves_exact(spectrum_of(s["m64"]))["new_mean"]) > 0.1


def test_curves_text_is_pinned(tmp_path):
    """the exact text, on the header's example"""
    spec = [[1, 1, 1, 0, 1], [2, 0, 0, 1, 1], [2, 1, 0, 0, 1]]
    ids = ["A", "B", "C", "D"]
    text = pr.spectrum_text(ids, 1, spec)
    assert text == ("# kmx pan spectrum\n# samples: 4\n# min_abund: 1\n# id: A\n# id: B\n# id: C\n# id: D\nr\trows\tfirst\tgap\n"
                    "0\t1\t2\t2\n1\t1\t0\t1\n2\t1\t0\t0\n3\t0\t1\t0\n4\t1\t1\t1\n")
    (tmp_path / "s.tsv").write_text(text)
    r = kmx("pan", "--from-spectrum", tmp_path / "s.tsv")
    assert r.returncode == 0, r.stderr
    # h = (1, 1, 1, 0, 1): pan(1) = 1/4 + 2/4 + 1, core(1) = the same, core(4) = 1, pan(4) = 3
    assert r.stdout == ("# kmx pan\n# samples: 4\n# rows: 4\n# min_abund: 1\n# heaps_alpha: 1.196628\n"
                        "m\tsample\tpan_mean\tcore_mean\tnew_mean\tpan_order\tcore_order\n"
                        "1\tA\t1.750000\t1.750000\t1.750000\t2\t2\n"
                        "2\tB\t2.333333\t1.166667\t0.583333\t2\t1\n"
                        "3\tC\t2.750000\t1.000000\t0.416667\t2\t1\n"
                        "4\tD\t3.000000\t1.000000\t0.250000\t3\t1\n")
    assert pr.shared_text(["D", "A"], [3, 0], [[0, 0, 0, 0], [1, 0, 0, 1], [1, 0, 0, 1]]) == "r\tD\tA\n0\t0\t0\n1\t1\t1\n2\t1\t1\n"


def test_usage_is_pinned():
    r = kmx("pan")
    assert r.returncode == 1 and r.stdout == "" and "usage: " + USAGE_RUN in r.stderr and "       " + USAGE_FROM in r.stderr
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert USAGE_RUN in readme and USAGE_FROM in readme


@pytest.mark.parametrize("edit,word", [
    (lambda t: t.replace("# samples: 4\n", ""), "samples"),
    (lambda t: t.replace("# min_abund: 1\n", ""), "min_abund"),
    (lambda t: t.replace("# id: C\n", ""), "id lines"),
    (lambda t: t.replace("r\trows\tfirst\tgap\n", "r\trows\n"), "column line"),
    (lambda t: t.replace("3\t0\t1\t0\n", ""), "expected r = 3"),
    (lambda t: t + "5\t0\t0\t0\n", "more than M + 1"),
    (lambda t: t.replace("4\t1\t1\t1\n", ""), "ends before"),
    (lambda t: t.replace("2\t1\t0\t0\n", "2\t1\tx\t0\n"), "expected a number"),
    (lambda t: t.replace("2\t1\t0\t0\n", "2\t-1\t0\t0\n"), "expected a number"),
    (lambda t: t.replace("2\t1\t0\t0\n", "2\t1\t0\n"), "four columns"),
    (lambda t: t.replace("2\t1\t0\t0\n", "2\t2\t0\t0\n"), "do not count the same rows"),
    (lambda t: t.replace("# samples: 4", "# samples: 0"), "sample count"),
    (lambda t: t.replace("# min_abund: 1", "# min_abund: 0"), "min_abund"),
    (lambda t: "", "ends before"),
])
def test_a_malformed_spectrum_is_refused(edit, word, tmp_path):
    text = pr.spectrum_text(["A", "B", "C", "D"], 1, [[1, 1, 1, 0, 1], [2, 0, 0, 1, 1], [2, 1, 0, 0, 1]])
    (tmp_path / "s.tsv").write_text(edit(text))
    r = kmx("pan", "--from-spectrum", tmp_path / "s.tsv", "--output", tmp_path / "out")
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "" and word in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out")
    r = kmx("pan", "--from-spectrum", tmp_path / "nothing.tsv")
    assert r.returncode == 1 and "nothing.tsv" in r.stderr and r.stdout == ""
    for extra in (("--samples", "x"), ("--gpus", 2), ("--min-abund", 2), ("--spectrum", "y"), ("--shared", "z"), ("--run", "w")):
        r = kmx("pan", "--from-spectrum", tmp_path / "s.tsv", *extra)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", extra


# ---- header, binding, sources -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_pan_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"PAN_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no PAN_EXPORTS"
    bound = set(re.findall(r'"(kmx_pan_\w+)"', listed.group(1)))
    want = {"kmx_pan_dev", "kmx_pan_host"} | {"kmx_pan_result_" + s for s in ("wait", "spectrum_dev", "shared_dev", "copy_spectrum", "copy_shared", "kernel_ms",
                                                                              "kernel_parts_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert "kmx_pan_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]      # the opening list of entry points
    assert "/* -------------------------------------------------------------------- pan */" in hdr
    assert re.search(r"#define KMX_PAN_SHARED 1u\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_pan_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == ["key_words", "mode", "n_cols", "n_use", "rows", "n_rows", "cols", "min_abund", "flags", "spectrum", "shared"]
    struct_src = re.search(r"class KmxPanTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    for name in ("KmxPanTask", "PanResult", "PanOutput", "def pan(", "def pan_dev("):
        assert name in src, name
    # the worked example stands in the header
    for text in ("(1,0,2,0)  rec 2, first 0, gap 1", "spectrum[0] = (1,1,1,0,1), spectrum[1] = (2,0,0,1,1), spectrum[2] = (2,1,0,0,1)",
                 "shared[1] = (0,0,0,1), shared[2] = (1,0,1,0), shared[4] = (1,1,1,1)"):
        assert text in hdr, text


def test_library_and_binding_structures():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert so.kmx_version() == 2
    assert len(lib.PAN_EXPORTS) == 11
    for name in lib.PAN_EXPORTS:
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxPanTask) == 64 and lib.KmxPanTask.cols.offset == 32 and lib.KmxPanTask.spectrum.offset == 48 and lib.PAN_SHARED == 1
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "pan.hip")).read()
    assert "static_assert(sizeof(kmx_pan_task) == 64" in src
    assert f"PN_LDS_WORDS = {3 * (pr.LDS_MAX_M + 1)};" in src


def test_pan_hip_has_knobs_of_its_own():
    csrc = os.path.join(ROOT, "kmtricks_amd", "csrc")
    src = open(os.path.join(csrc, "pan.hip")).read()
    for word in ("kmx_plan_cus", "kmx_grid_cap", "KMX_PLAN_CUS", "KMX_MAX_GRID"):
        assert word not in src, word
    assert 'kmx_env_cus("KMX_PAN_CUS", ctx)' in src and 'kmx_env_grid("KMX_PAN_GRID", dflt)' in src
    assert "pan.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "kmx_pan.cpp" in open(os.path.join(ROOT, "kmtricks_amd", "host", "Makefile")).read()
    curves = open(os.path.join(ROOT, "kmtricks_amd", "host", "kmx_pan_curves.hpp")).read()
    assert "lgamma" not in curves.replace("no lgamma", "") and "hip" not in curves.lower()


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output, nothing written ---------------
MODES = ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxpan")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in MODES:
        rmode = dr.KINDS[mode][5]
        bodies = [pr.make_body(p, 10, 3, 1, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    return dict(dir=d, runs=out, ids=ids, k=k)


def refused(tmp_path, *args, word=None):
    outs = [tmp_path / n for n in ("out.tsv", "spec.tsv", "shared.tsv")]
    r = kmx("pan", *args, "--output", outs[0], "--spectrum", outs[1], "--shared", outs[2])
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert word is None or word in r.stderr, (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert not any(os.path.exists(p) for p in outs), "a refusal wrote a file"
    r = kmx("pan", *args)
    assert r.returncode == 1 and r.stdout == ""


def samples_file(tmp_path, text):
    with open(tmp_path / "s.txt", "w") as f:
        f.write(text)
    return tmp_path / "s.txt"


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_bad_options(runs, tmp_path, mode):
    run = runs["runs"][mode]
    refused(tmp_path, "--run", tmp_path / "nothing", word="not a kmtricks runtime directory")
    refused(tmp_path, "--run", run, "--frobnicate")
    refused(tmp_path, "--run", run, "--min-abund", 0, word="--min-abund")
    refused(tmp_path, "--run", run, "--min-abund", "-1", word="--min-abund")
    refused(tmp_path, "--run", run, "--min-abund", 2 ** 32, word="--min-abund")
    for g in (0, 17, "two"):
        refused(tmp_path, "--run", run, "--gpus", g, word="--gpus")
    refused(tmp_path, "--run", run, "--batch-mb", "lots", word="--batch-mb")
    refused(tmp_path, "--run", run, "--samples")
    if mode.split(":")[1] == "pa":
        refused(tmp_path, "--run", run, "--min-abund", 2, word="--min-abund")


@pytest.mark.parametrize("text,word", [
    ("A\nD\n", "D is not in the run"),           # an id that is not in the fof
    ("A\nB\nA\n", "A is named twice"),           # a duplicate
    ("A B\n", "expected one sample id"),         # two words
    ("", "names no sample"),                     # an empty list
    ("\n \n", "names no sample"),
])
def test_driver_refuses_bad_sample_lists(runs, tmp_path, text, word):
    for mode in ("kmer:count:bin", "hash:pa:bin"):
        refused(tmp_path, "--run", runs["runs"][mode], "--samples", samples_file(tmp_path, text), word=word)
    refused(tmp_path, "--run", runs["runs"]["kmer:pa:bin"], "--samples", tmp_path / "nothing.txt", word="nothing.txt")


def test_driver_refuses_modes_it_does_not_read(runs, tmp_path):
    body = pr.make_body(1, 4, 3, 1, COUNT)
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text", "kmer:pa:text", "hash:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused(tmp_path, "--run", root, word=said)


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
    refused(tmp_path, "--run", d, word=f"matrix_1.{ext}")
    d = variant("gone")          # a missing matrix
    os.remove(d / f1)
    refused(tmp_path, "--run", d, word=f"matrix_1.{ext}")
    d = variant("cols")          # a header of another number of columns than the fof has samples
    with open(d / f1, "r+b") as f:
        f.seek(cols_at); f.write(struct.pack("<I", 4))
    refused(tmp_path, "--run", d, word=f"matrix_1.{ext}")
    d = variant("magic")         # another kind of file under the name
    with open(d / f1, "r+b") as f:
        f.seek(13); f.write(struct.pack("<Q", 0x1234))
    refused(tmp_path, "--run", d, word="Invalid file format")
    d = variant("nofof")         # a fof with a sample more than the matrices have columns
    with open(d / "kmtricks.fof", "a") as f:
        f.write("D : /nowhere/D.fasta\n")
    refused(tmp_path, "--run", d, word=f"matrix_0.{ext}")
    d = variant("noopt")
    os.remove(d / "options.txt")
    refused(tmp_path, "--run", d, word="options.txt")
    d = variant("noparts")       # the partition count's file
    os.remove(d / ("repartition_gatb/repartition.minimRepart" if mode.startswith("kmer") else "hash.info"))
    refused(tmp_path, "--run", d)
