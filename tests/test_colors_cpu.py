"""CPU-only: tests/colors_ref.py (the judge of `kmx colors`) against the example the header works by hand, its two roads against each
other, the identities of the header (the one that ties the class table to `kmx pan`'s spectrum included), the driver's table text, sort
order and --ids files on a hand-made table, the new symbols of the C ABI as the header and the binding name them, and the refusals of
`kmx colors` that come before any device is asked for, on run directories written by hand."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dist_ref as dr
import colors_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = cr.MODE_COUNT, cr.MODE_PA
USAGE = ("kmx colors --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
         "[--min-abund INT] [--top INT] [--output FILE] [--ids DIR] [--gpus INT] [--batch-mb INT] [-v]")


def both(body, N, kw, mode, cols=None, a=1):
    """the two roads, equal -> (C, ids, first, sizes, patterns) as lists of Python integers"""
    py = cr.colors_expected_py(body, N, kw, mode, cols, a)
    C, ids, first, sizes, patterns = cr.colors_expected_np(body, N, kw, mode, cols, a)
    got = (C, [int(x) for x in ids], [int(x) for x in first], [int(x) for x in sizes], [[int(w) for w in p] for p in patterns])
    assert got == py.as_lists(), (N, kw, mode, cols, a)
    assert patterns.shape == (C, py.W) and patterns.dtype == np.uint64 and ids.dtype == first.dtype == sizes.dtype == np.uint32
    return got


def count_rows(rows, kw=1):
    return b"".join(bytes(range(1, 8 * kw + 1)) + struct.pack(f"<{len(r)}I", *r) for r in rows)


EXAMPLE = [(1, 0, 2, 0), (0, 0, 0, 5), (3, 0, 1, 0), (0, 0, 0, 0), (0, 0, 0, 1), (7, 0, 9, 0)]


def test_worked_example():
    """the example of include/kmx.h, section colors, as literals: all three variants"""
    body = count_rows(EXAMPLE)
    assert both(body, 4, 1, COUNT) == (3, [0, 1, 0, 2, 1, 0], [0, 1, 3], [3, 2, 1], [[5], [8], [0]])
    C, ids, first, sizes, patterns = both(body, 4, 1, COUNT, a=2)
    assert (C, ids, sizes, patterns) == (5, [0, 1, 2, 3, 3, 4], [1, 1, 1, 2, 1], [[4], [8], [1], [0], [5]])
    assert both(body, 4, 1, COUNT, cols=(2, 0)) == (2, [0, 1, 0, 1, 1, 0], [0, 1], [3, 3], [[3], [0]])
    # the same rows as presence/absence bits, every padding bit set
    pa = b"".join(bytes(8) + bytes([sum((v > 0) << i for i, v in enumerate(r)) | 0xF0]) for r in EXAMPLE)
    assert both(pa, 4, 1, PA) == both(body, 4, 1, COUNT)
    # the header says what the test says
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for text in ("(1,0,2,0) (0,0,0,5) (3,0,1,0) (0,0,0,0) (0,0,0,1) (7,0,9,0)", "C = 3, patterns = (5, 8, 0), first = (0, 1, 3), size = (3, 2, 1), ids = (0,1,0,2,1,0)",
                 "C = 5, patterns = (4, 8, 1, 0, 5), size = (1,1,1,2,1), ids = (0,1,2,3,3,4)", "C = 2, patterns = (3, 0), first = (0, 1), size = (3, 3), ids = (0,1,0,1,1,0)"):
        assert text in hdr, text


def row_pattern_of(body, N, kw, mode, cols, a):
    """a row's W words, straight from the payload (a third, tiny restatement for the identity 'the row first[c] has patterns[c]')"""
    pay = dr.split_payload(body, N, kw, mode)
    listed = list(range(N)) if cols is None else [int(c) for c in cols]
    W = (len(listed) + 63) // 64

    def of(r):
        bits = sum(int(pay[r][c] >= a if mode == COUNT else pay[r][c]) << j for j, c in enumerate(listed))
        return [(bits >> (64 * w)) & (2 ** 64 - 1) for w in range(W)]
    return of


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_the_two_roads_agree_and_the_identities_hold(mode):
    """N 1 ... 130, every padding bit set, fills 0 / 0.02 / 0.5 / 1, counts of 2^32 - 1, lists of every kind; the identities, the one
    against pan_ref's spectrum[0] on the same task included"""
    for N in range(1, 131):
        fill = (0.0, 0.02, 0.5, 1.0)[N % 4]
        kw = 1 + N % 4
        rows = 1 + (N * 7) % 23
        body = cr.make_body(700 + N, rows, N, kw, mode, fill=fill, pad_ones=True, maxed=0.2, lo=1, hi=4)
        kind = cr.KINDS[N % len(cr.KINDS)]
        cols = cr.make_cols(kind, N, N)
        M = N if cols is None else len(cols)
        for a in ((1, 2, cr.U32)[N % 3], 1) if mode == COUNT else (1,):
            C, ids, first, sizes, patterns = both(body, N, kw, mode, cols, a)
            spec = cr.pan_expected_np(body, N, kw, mode, cols, a)[0]
            cr.check_identities(C, ids, first, sizes, patterns, rows, M, row_pattern_of(body, N, kw, mode, cols, a), spec[0])


def test_the_two_roads_agree_on_the_gpu_cases():
    """the list tests/test_colors_gpu.py walks (the Python road where rows x M stays small), with the identities"""
    n = 0
    for c in cr.gpu_cases():
        for a, exp in c.expected.items():
            C, ids, first, sizes, patterns = exp
            spec0 = cr.pan_expected_np(c.body, c.n_cols, c.key_words, c.mode, c.cols, a)[0][0]
            cr.check_identities(C, ids, first, sizes, patterns, c.n_rows, c.n_use, spectrum0=spec0)
            if c.n_rows * c.n_use <= 70000:
                both(c.body, c.n_cols, c.key_words, c.mode, c.cols, a)
                n += 1
    assert n >= 40


def test_the_sweep_covers_what_it_says():
    """every value of the issue's table appears in the list tests/test_colors_gpu.py walks, in both modes, and the structures are what
    they say"""
    cases = cr.gpu_cases()
    for mode in (COUNT, PA):
        mine = [c for c in cases if c.mode == mode]
        assert {c.n_cols for c in mine} >= set(cr.COLUMNS)
        assert {c.n_rows for c in mine} >= set(cr.ROWS)
        assert {c.key_words for c in mine} == {1, 2, 3, 4}
        assert {c.name.split("-")[2] for c in mine} >= set(cr.KINDS)
        assert {c.name.split("-")[5] for c in mine} >= set(cr.STRUCTURES)
        assert {(c.n_use + 63) // 64 for c in mine} >= {1, 2, 3, 5, 17}      # W: one word, two, many
    assert {a for c in cases for a in c.abunds} == {1, 2, cr.U32}
    assert cr.case("c-9-none-r4200-k1-one-long").expected[1][0] == 1
    assert cr.case("p-65-reversed-r4200-k1-distinct-long").expected[1][0] == 4200
    assert cr.case("c-40-none-r4200-k1-distinct-long").expected[1][0] == 4200
    C, ids, first, sizes, _ = cr.case("p-130-scattered-r4200-k1-skewed-long").expected[1]
    assert sizes[0] + sizes[1] > 0.85 * 4200 and C > 300 and max(sizes[2:]) <= 2      # 60 % + 30 %, singletons after
    C, ids, _, sizes, _ = cr.case("c-64-none-r4200-k1-alternate-long").expected[1]
    assert C == 2 and list(ids[:4]) == [0, 1, 0, 1] and list(sizes) == [2100, 2100]
    c = cr.case("p-257-scattered-r4200-k1-last-long")
    C, _, _, _, patterns = c.expected[1]
    assert C == 2 and (patterns[0] ^ patterns[1]).tolist() == [0] * ((c.n_use - 1) // 64) + [1 << ((c.n_use - 1) % 64)]      # the LAST listed column alone


# ---- the driver's texts ------------------------------------------------------------------------------------------------------------
def test_table_text_sort_order_and_top():
    """rows descending, ties by the 0/1 string ascending; --top cuts the lines, not the counts; ids files carry the rank in the full table"""
    ids = ["A", "B", "C"]
    table = {(0b101,): 7, (0b000,): 7, (0b010,): 9, (0b111,): 1, (0b100,): 7}
    assert cr.colors_text(ids, 2, table) == ("# kmx colors\n# samples: 3\n# rows: 31\n# classes: 5\n# min_abund: 2\n# shown: 5\n"
                                             "rank\trows\trec\tpattern\tsamples\n"
                                             "0\t9\t1\t010\tB\n"
                                             "1\t7\t0\t000\t-\n"
                                             "2\t7\t1\t001\tC\n"
                                             "3\t7\t2\t101\tA,C\n"
                                             "4\t1\t3\t111\tA,B,C\n")
    top = cr.colors_text(ids, 2, table, top=2)
    assert top == ("# kmx colors\n# samples: 3\n# rows: 31\n# classes: 5\n# min_abund: 2\n# shown: 2\nrank\trows\trec\tpattern\tsamples\n0\t9\t1\t010\tB\n1\t7\t0\t000\t-\n")
    assert "# shown: 5\n" in cr.colors_text(ids, 2, table, top=9) and cr.colors_text(ids, 2, table, top=0).endswith("# shown: 0\nrank\trows\trec\tpattern\tsamples\n")
    head, rows = cr.parse_colors(top)
    assert head == dict(samples="3", rows="31", classes="5", min_abund="2", shown="2") and rows == [(0, 9, 1, "010", "B"), (1, 7, 0, "000", "-")]
    files = cr.ids_files(table, [[(0b111,), (0b010,)], [], [(0b100,), (0b100,), (0b000,)]], 3)
    assert files == [struct.pack("<2I", 4, 0), b"", struct.pack("<3I", 2, 2, 1)]
    # a pattern of more than one word: ordinal 64 is bit 0 of word 1
    assert cr.bits_text((1, 1), 66) == "1" + "0" * 63 + "10"
    # two partitions' tables merge by pattern
    a = cr.colors_expected_np(count_rows(EXAMPLE), 4, 1, COUNT)
    b = cr.colors_expected_np(count_rows(EXAMPLE[3:] + [(0, 1, 0, 0)]), 4, 1, COUNT)
    merged, row_patterns = cr.merged_table([a, b])
    assert merged == {(5,): 4, (8,): 3, (0,): 2, (2,): 1} and row_patterns[1] == [(0,), (8,), (5,), (2,)]


def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def test_usage_is_pinned():
    r = kmx("colors")
    assert r.returncode == 1 and r.stdout == "" and "usage: " + USAGE in r.stderr
    assert USAGE in open(os.path.join(ROOT, "README.md")).read()
    r = kmx()
    assert r.returncode == 1 and "kmx colors --run <dir> [options]" in r.stderr


# ---- header, binding, sources -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_colors_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"COLORS_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no COLORS_EXPORTS"
    bound = set(re.findall(r'"(kmx_colors_\w+)"', listed.group(1)))
    want = {"kmx_colors_dev", "kmx_colors_host"} | {"kmx_colors_result_" + s for s in ("wait", "n_classes", "ids_dev", "copy_ids", "copy_first", "copy_sizes",
                                                                                      "copy_patterns", "kernel_ms", "kernel_parts_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert "kmx_colors_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]      # the opening list of entry points
    assert "/* ----------------------------------------------------------------- colors */" in hdr
    assert re.search(r"KMX_E_INTERNAL = -6\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_colors_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == ["key_words", "mode", "n_cols", "n_use", "rows", "n_rows", "cols", "min_abund", "flags"]
    struct_src = re.search(r"class KmxColorsTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    for name in ("KmxColorsTask", "ColorsResult", "ColorsOutput", "def colors(", "def colors_dev("):
        assert name in src, name
    # the scratch per row and the algorithmic bytes are stated
    assert "PER ROW 8 * W + 24 bytes" in hdr and "2 * n_rows * (8 * W + 8)" in hdr


def test_library_and_binding_structures():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert so.kmx_version() == 2
    assert len(lib.COLORS_EXPORTS) == 13
    for name in lib.COLORS_EXPORTS:
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxColorsTask) == 48 and lib.KmxColorsTask.cols.offset == 32 and lib.KmxColorsTask.flags.offset == 44 and lib.E_INTERNAL == -6
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "colors.hip")).read()
    assert "static_assert(sizeof(kmx_colors_task) == 48" in src


def test_colors_hip_has_knobs_of_its_own():
    csrc = os.path.join(ROOT, "kmtricks_amd", "csrc")
    src = open(os.path.join(csrc, "colors.hip")).read()
    for word in ("kmx_plan_cus", "kmx_grid_cap", "KMX_PLAN_CUS", "KMX_MAX_GRID", "KMX_PAN_"):
        assert word not in src, word
    for read in ('kmx_env_cus("KMX_COLORS_CUS", ctx)', 'kmx_env_grid("KMX_COLORS_GRID", dflt)', 'kmx_env_int("KMX_COLORS_HASH_BITS")'):
        assert read in src, read
    assert "__threadfence" not in src and "__atomic_load" not in src      # what is compared was written by the launch before
    assert "colors.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "kmx_colors.cpp" in open(os.path.join(ROOT, "kmtricks_amd", "host", "Makefile")).read()


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output, nothing written ---------------
MODES = ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxcolors")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in MODES:
        rmode = dr.KINDS[mode][5]
        bodies = [cr.make_body(p, 10, 3, 1, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    return dict(dir=d, runs=out, ids=ids, k=k)


def refused(tmp_path, *args, text=None):
    outs = [tmp_path / "out.tsv", tmp_path / "ids"]
    r = kmx("colors", *args, "--output", outs[0], "--ids", outs[1])
    assert r.returncode == 1 and r.stderr.startswith("[error] ") and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert text is None or r.stderr.startswith("[error] " + text), (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert not any(os.path.exists(p) for p in outs), "a refusal wrote a file"
    r = kmx("colors", *args)
    assert r.returncode == 1 and r.stdout == ""


def samples_file(tmp_path, text):
    with open(tmp_path / "s.txt", "w") as f:
        f.write(text)
    return tmp_path / "s.txt"


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_bad_options(runs, tmp_path, mode):
    run = runs["runs"][mode]
    refused(tmp_path, "--run", tmp_path / "nothing", text=f"{tmp_path / 'nothing'} is not a kmtricks runtime directory.\n")
    refused(tmp_path, "--run", run, "--frobnicate", text="unknown option --frobnicate\nusage: " + USAGE)
    refused(tmp_path, "--run", run, "--min-abund", 0, text="--min-abund must be at least 1\n")
    refused(tmp_path, "--run", run, "--min-abund", "-1", text="bad number for --min-abund: -1\n")
    refused(tmp_path, "--run", run, "--min-abund", 2 ** 32, text="--min-abund does not fit 32 bits\n")
    for g in (0, 17):
        refused(tmp_path, "--run", run, "--gpus", g, text="--gpus must be in [1, 16]\n")
    refused(tmp_path, "--run", run, "--gpus", "two", text="bad number for --gpus: two\n")
    refused(tmp_path, "--run", run, "--batch-mb", "lots", text="bad number for --batch-mb: lots\n")
    refused(tmp_path, "--run", run, "--top", "-3", text="bad number for --top: -3\n")
    refused(tmp_path, "--run", run, "--samples")      # (here the option swallows the --output that refused() appends)
    r = kmx("colors", "--run", run, "--samples")
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("[error] missing value for --samples\nusage: " + USAGE)
    refused(tmp_path, "--top", 3, text="--run is required\nusage: " + USAGE)
    if mode.split(":")[1] == "pa":
        refused(tmp_path, "--run", run, "--min-abund", 2, text=f"--min-abund above 1 needs counts: {run} was made with {mode}\n")


@pytest.mark.parametrize("text,word", [
    ("A\nD\n", "line 2: sample D is not in the run's kmtricks.fof\n"),      # an id that is not in the fof
    ("A\nB\nA\n", "line 3: sample A is named twice\n"),                       # a duplicate
    ("A B\n", "line 1: expected one sample id\n"),                            # two words
    ("", "names no sample\n"),                                                 # an empty list
    ("\n \n", "names no sample\n"),
])
def test_driver_refuses_bad_sample_lists(runs, tmp_path, text, word):
    for mode in ("kmer:count:bin", "hash:pa:bin"):
        path = samples_file(tmp_path, text)
        refused(tmp_path, "--run", runs["runs"][mode], "--samples", path, text=f"{path} {word}")
    refused(tmp_path, "--run", runs["runs"]["kmer:pa:bin"], "--samples", tmp_path / "nothing.txt", text=f"Unable to read at {tmp_path / 'nothing.txt'}\n")


def test_driver_refuses_modes_it_does_not_read(runs, tmp_path):
    body = cr.make_body(1, 4, 3, 1, COUNT)
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text", "kmer:pa:text", "hash:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused(tmp_path, "--run", root, text="kmx colors needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; "
                                               f"{root} was made with {said}\n")


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_files_that_do_not_fit(runs, mode, tmp_path):
    ext, hdr, magic, cols_at, kw, rmode = dr.KINDS[mode]
    src = runs["runs"][mode]
    f1 = os.path.join("matrices", f"matrix_1.{ext}")
    stride = dr.row_bytes(1, 3, rmode)

    def variant(name):
        shutil.copytree(src, tmp_path / name)
        return tmp_path / name

    d = variant("cut")           # a truncated body: no whole number of rows
    with open(d / f1, "r+b") as f:
        f.truncate(os.path.getsize(d / f1) - 1)
    refused(tmp_path, "--run", d, text=f"truncated matrix (its body is no whole number of rows of {stride} bytes): {d / f1}\n")
    d = variant("gone")          # a missing matrix
    os.remove(d / f1)
    refused(tmp_path, "--run", d, text=f"Unable to read at {d / f1}\n")
    d = variant("cols")          # a header of another number of columns than the fof has samples
    with open(d / f1, "r+b") as f:
        f.seek(cols_at); f.write(struct.pack("<I", 4))
    refused(tmp_path, "--run", d, text=f"{d / f1} has rows of 4 columns, the run's kmtricks.fof has 3 samples\n")
    d = variant("magic")         # another kind of file under the name
    with open(d / f1, "r+b") as f:
        f.seek(13); f.write(struct.pack("<Q", 0x1234))
    refused(tmp_path, "--run", d, text=f"Invalid file format: {d / f1}\n")
    d = variant("nofof")         # a fof with a sample more than the matrices have columns
    with open(d / "kmtricks.fof", "a") as f:
        f.write("D : /nowhere/D.fasta\n")
    refused(tmp_path, "--run", d, text=f"{d / 'matrices' / ('matrix_0.' + ext)} has rows of 3 columns, the run's kmtricks.fof has 4 samples\n")
    d = variant("noopt")
    os.remove(d / "options.txt")
    refused(tmp_path, "--run", d, text=f"Unable to read at {d}/options.txt\n")
    d = variant("noparts")       # the partition count's file
    os.remove(d / ("repartition_gatb/repartition.minimRepart" if mode.startswith("kmer") else "hash.info"))
    refused(tmp_path, "--run", d)
