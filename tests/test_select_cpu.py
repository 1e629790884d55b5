"""CPU-only: tests/select_ref.py (the judge of `kmx select`) against the examples the header works by hand, its two roads against each
other over the sweep the GPU test sends, the condition under which that sweep shows anything (keep-none, keep-all and a proper subset for
every pair of modes), the new symbols of the C ABI as the header and the binding name them, and the refusals of `kmx select` that come
before any device is asked for, on run directories written by hand."""
import collections
import ctypes
import os
import re
import shutil
import struct
import subprocess
import numpy as np
import pytest

import dist_ref as dr
import select_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = sr.MODE_COUNT, sr.MODE_PA


def both(body, N, kw, mode, **args):
    """the two roads, equal -> (body bytes, [(row, rec)])"""
    a, b = sr.select_expected_np(body, N, kw, mode, **args), sr.select_expected_py(body, N, kw, mode, **args)
    assert a[0] == b[0] and [(int(x["row"]), int(x["rec"])) for x in a[1]] == b[1], args
    return b


def test_worked_examples():
    """the examples of include/kmx.h, section select, as literals"""
    key = bytes(range(1, 9))
    row = key + struct.pack("<5I", 0, 3, 10, 1, 7)
    cols = (4, 2, 1)
    assert both(row, 5, 1, COUNT, cols=cols, min_abund=3) == (key + struct.pack("<3I", 7, 10, 3), [(0, 3)])
    assert both(row, 5, 1, COUNT, cols=cols, min_abund=5) == (key + struct.pack("<3I", 7, 10, 3), [(0, 2)])
    assert both(row, 5, 1, COUNT, cols=cols, min_abund=5, zero_below=True) == (key + struct.pack("<3I", 7, 10, 0), [(0, 2)])
    assert both(row, 5, 1, COUNT, cols=cols, min_abund=5, out_mode=PA) == (key + b"\x03", [(0, 2)])
    assert both(row, 5, 1, COUNT, cols=cols, min_abund=3, out_mode=PA) == (key + b"\x07", [(0, 3)])
    # rec over the selected columns only: column 3 holds the row, the list does not name it
    lone = key + struct.pack("<5I", 0, 0, 0, 9, 0)
    assert both(lone, 5, 1, COUNT, cols=cols, min_rec=1) == (b"", [])
    assert both(lone, 5, 1, COUNT, cols=cols, min_rec=0) == (key + bytes(12), [(0, 0)])
    # the range: min_rec above max_rec keeps nothing, max_rec at M and above is no bound
    two = row + lone
    assert both(two, 5, 1, COUNT, cols=cols, min_rec=2, max_rec=1)[1] == []
    assert both(two, 5, 1, COUNT, cols=cols, min_rec=0, max_rec=2)[1] == [(1, 0)]
    assert both(two, 5, 1, COUNT, cols=cols, min_rec=0, max_rec=3)[1] == both(two, 5, 1, COUNT, cols=cols, max_rec=2 ** 32 - 1)[1] == [(0, 3), (1, 0)]
    # presence/absence rows, every padding bit set: the padding never reaches a result, and the result's own padding is 0
    pa = key + bytes([0b10110 | 0xE0])      # columns 1, 2 and 4
    assert both(pa, 5, 1, PA, cols=cols) == (key + b"\x07", [(0, 3)])
    assert both(pa, 5, 1, PA, cols=(0, 4, 3)) == (key + b"\x02", [(0, 1)])
    assert both(pa, 5, 1, PA) == (key + bytes([0b10110]), [(0, 3)])
    assert sr.SELECT_REC.itemsize == 8


def test_the_two_roads_agree_over_the_sweep():
    """every body and parameter set that tests/test_select_gpu.py sends: numpy over whole columns against Python a bit at a time"""
    cases = sr.gpu_cases()
    assert len({c.name for c in cases}) == len(cases) >= 50
    for c in cases:
        for a in sorted({r["min_abund"] for r in c.runs}):
            rows = sr.rows_py(c.body, c.n_cols, c.key_words, c.mode, c.cols, a)
            for r, (body, recs) in zip(c.runs, c.expected):
                if r["min_abund"] == a:
                    b2, r2 = sr.assemble_py(rows, c.mode, r["out_mode"], a, r["min_rec"], r["max_rec"], r["zero_below"])
                    assert b2 == body and r2 == [(int(x["row"]), int(x["rec"])) for x in recs], (c.name, r)
        if c.mode == PA and c.n_cols % 8:      # the input's padding bits are all set: one that reached a result would show in rec
            rb = dr.row_bytes(c.key_words, c.n_cols, c.mode)
            assert c.n_rows == 0 or (np.asarray(c.body).reshape(-1, rb)[:, -1] >> (c.n_cols % 8)).min() == (0xFF >> (c.n_cols % 8))
            assert all(int(recs["rec"].max(initial=0)) <= c.n_out for _, recs in c.expected)


def test_the_sweep_covers_what_it_says():
    """every value of the issue's table appears, every (column shape, mode pair) appears, and for every mode pair the reference alone
    shows keep-none, keep-all and a proper subset between 10 % and 90 %: the GPU test cannot pass on trivial keep sets"""
    cases = sr.gpu_cases()
    seen = collections.defaultdict(set)
    shares = collections.defaultdict(set)
    for c in cases:
        pair = (c.mode, c.out_mode)
        kind = c.name.split("-")[2] if not c.name.endswith("subset") else "perm"
        seen["N"].add(c.n_cols); seen["M"].add(c.n_out); seen["rows"].add(c.n_rows); seen["kw"].add(c.key_words)
        seen["shape"].add((c.n_cols, c.n_out, c.cols is None, pair))
        seen["kind"].add("none" if c.cols is None else kind)
        for r, (body, recs) in zip(c.runs, c.expected):
            seen["a"].add(r["min_abund"]); seen["zb"].add(r["zero_below"])
            seen["range"].add("none" if r["max_rec"] is not None and r["min_rec"] > r["max_rec"] else
                              ("all" if r["min_rec"] == 0 else "some") + ("" if r["max_rec"] is None or r["max_rec"] >= c.n_out else "-bounded"))
            if c.n_rows >= 63:
                f = len(recs) / c.n_rows
                shares[pair].add("none" if f == 0 else "all" if f == 1 else "subset" if 0.1 <= f <= 0.9 else "other")
        if c.mode == COUNT and c.n_rows:
            seen["maxed"].add(bool((dr.split_payload(c.body, c.n_cols, c.key_words, c.mode) == sr.U32).any()))
    assert seen["N"] == {1, 7, 8, 9, 63, 64, 65, 130, 520, 2049, 2100}
    # count columns beyond the 2048 whose selection a lane keeps in a register: for both output modes, lists that take such a column and
    # lists that leave one, and a run that keeps a proper subset of the rows
    for N, kind, M in sr.WIDE_COUNT_SHAPES:
        for pair in sr.MODE_PAIRS[:2]:
            c = next(x for x in cases if x.n_cols == N and x.n_out == M and (x.mode, x.out_mode) == pair and f"-{kind}-" in x.name)
            far = set(range(2048, N))
            assert far & set(c.cols.tolist()) or N == 2049, c.name
            assert 0.1 <= len(c.expected[-1][1]) / c.n_rows <= 0.9, c.name
    took = {N: [bool(set(range(2048, N)) & set(c.cols.tolist())) for c in cases if c.n_cols == N] for N in (2049, 2100)}
    left = {N: [bool(set(range(2048, N)) - set(c.cols.tolist())) for c in cases if c.n_cols == N] for N in (2049, 2100)}
    assert all(any(took[N]) and any(left[N]) for N in (2049, 2100)), (took, left)
    assert seen["M"] >= {1, 7, 8, 9, 63, 64, 65, 520}
    assert seen["rows"] >= {0, 1, 63, 64, 65, 255, 256, 257, 4200}
    assert seen["kw"] == {1, 2, 3, 4} and seen["a"] == {1, 2, sr.U32} and seen["zb"] == {False, True} and True in seen["maxed"]
    assert seen["range"] >= {"all", "some", "some-bounded", "none"}
    assert seen["kind"] == {"none", "identity", "reversed", "every", "perm", "one"}
    for N, kind, M in sr.COLUMN_SHAPES:
        for pair in sr.MODE_PAIRS:
            assert (N, M, kind == "none", pair) in seen["shape"], (N, kind, M, pair)
    for pair in sr.MODE_PAIRS:
        assert shares[pair] >= {"none", "all", "subset"}, (pair, shares[pair])
    fills = {c.name.rsplit("-f", 1)[1] for c in cases if "-f" in c.name}
    assert fills == {"0.0", "0.02", "0.5", "1.0"}


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_select_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"SELECT_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no SELECT_EXPORTS"
    bound = set(re.findall(r'"(kmx_select_\w+)"', listed.group(1)))
    want = {"kmx_select_dev", "kmx_select_host"} | {"kmx_select_result_" + s for s in ("wait", "rows", "row_bytes", "body_bytes", "body_dev", "copy_body", "recs_dev",
                                                                                    "copy_recs", "kernel_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert "kmx_select_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]      # the opening list of entry points
    assert "/* ----------------------------------------------------------------- select */" in hdr
    assert re.search(r"#define KMX_SELECT_ZERO_BELOW 1u\b", hdr)
    # the binding's structure has the header's fields in the header's order
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_select_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    struct_src = re.search(r"class KmxSelectTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_select_rec;", hdr, re.S).group(1), flags=re.S)
    assert [d.split()[-1] for d in body.split(";") if d.strip()] == list(sr.SELECT_REC.names)
    for name in ("KmxSelectTask", "SelectResult", "SelectOutput", "SELECT_REC", "def select(", "def select_dev("):
        assert name in src, name


def test_library_and_binding_structures():
    """the built library has the symbols (kmx_version unchanged); the binding's structure has the C size; a record is 8 bytes"""
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert so.kmx_version() == 2
    assert len(lib.SELECT_EXPORTS) == 13
    for name in lib.SELECT_EXPORTS:
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxSelectTask) == 64 and lib.KmxSelectTask.cols.offset == 32 and lib.KmxSelectTask.min_abund.offset == 40
    assert lib.SELECT_REC.itemsize == 8 and lib.SELECT_REC == sr.SELECT_REC and lib.SELECT_ZERO_BELOW == 1


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output, nothing written ---------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


MODES = ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxselect")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in MODES:
        rmode = dr.KINDS[mode][5]
        bodies = [sr.make_body(p, 10, 3, 1, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    return dict(dir=d, runs=out, ids=ids, k=k)


def refused(tmp_path, *args, word=None, out=None):
    out = tmp_path / "out" if out is None else out
    before = sorted(os.listdir(out)) if os.path.isdir(out) else None
    r = kmx("select", *args, "--output", out)
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert word is None or word in r.stderr, (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert (sorted(os.listdir(out)) if os.path.isdir(out) else None) == before, "a refusal wrote under the output directory"


def samples_file(tmp_path, text):
    with open(tmp_path / "s.txt", "w") as f:
        f.write(text)
    return tmp_path / "s.txt"


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_bad_options(runs, tmp_path, mode):
    run = runs["runs"][mode]
    r = kmx("select", "--run", run)
    assert r.returncode == 1 and "--output" in r.stderr
    r = kmx("select", "--output", tmp_path / "o")
    assert r.returncode == 1 and "--run" in r.stderr and not os.path.exists(tmp_path / "o")
    refused(tmp_path, "--run", tmp_path / "nothing", word="not a kmtricks runtime directory")
    refused(tmp_path, "--run", run, "--frobnicate")
    for f in ("-0.1", "1.5", "nan", "half"):
        refused(tmp_path, "--run", run, "--min-frac", f, word="--min-frac")
        refused(tmp_path, "--run", run, "--max-frac", f, word="--max-frac")
    refused(tmp_path, "--run", run, "--min-rec", 1, "--min-frac", 0.5, word="--min-frac")
    refused(tmp_path, "--run", run, "--max-rec", 1, "--max-frac", 0.5, word="--max-frac")
    refused(tmp_path, "--run", run, "--min-rec", "-1", word="--min-rec")
    refused(tmp_path, "--run", run, "--min-abund", 0, word="--min-abund")
    refused(tmp_path, "--run", run, "--zero-below", "--pa", word="--zero-below")
    for g in (0, 17, "two"):
        refused(tmp_path, "--run", run, "--gpus", g, word="--gpus")
    if mode.split(":")[1] == "pa":
        refused(tmp_path, "--run", run, "--min-abund", 2, word="--min-abund")
        refused(tmp_path, "--run", run, "--zero-below", word="--zero-below")
    # the output's place: a directory with something in it, a file
    full = tmp_path / "full"
    os.makedirs(full / "matrices")
    refused(tmp_path, "--run", run, word="not an empty directory", out=full)
    with open(tmp_path / "file", "w") as f:
        f.write("x")
    refused(tmp_path, "--run", run, word="not an empty directory", out=tmp_path / "file")


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
    body = sr.make_body(1, 4, 3, 1, COUNT)
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
