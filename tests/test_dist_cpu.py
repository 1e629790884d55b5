"""CPU-only: tests/dist_ref.py (the judge of `kmx dist`) against the examples the header works by hand, its two roads against each other,
the driver's text produced from tables, the new symbols of the C ABI as the header and the binding name them, and the refusals of
`kmx dist` that come before any device is asked for, on run directories written by hand."""
import os
import re
import shutil
import struct
import subprocess
import numpy as np
import pytest

import dist_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA, BF = dr.MODE_COUNT, dr.MODE_PA, dr.MODE_BF


def both(body, N, kw, mode, mins=False):
    a, b = dr.dist_expected_py(body, N, kw, mode, mins), dr.dist_expected_np(body, N, kw, mode, mins)
    assert np.array_equal(np.array(a[0], np.uint64).reshape(N, N), b[0])
    if mins:
        assert np.array_equal(np.array(a[1], np.uint64).reshape(N, N), b[1])
    else:
        assert a[1] is None and b[1] is None
    return b


def test_worked_examples():
    """the examples of include/kmx.h, section dist, as literals"""
    key = bytes(8)
    pa = b"".join(key + bytes([b]) for b in (0b011, 0b101, 0b111, 0b000))
    inter, mins = both(pa, 3, 1, PA)
    assert inter.tolist() == [[3, 2, 2], [2, 2, 1], [2, 1, 2]]
    # every padding bit set, and no key (a Bloom matrix): the same table
    bf = bytes([0b011 | 0xF8, 0b101 | 0xF8, 0b111 | 0xF8, 0xF8])
    assert both(bf, 3, 0, BF)[0].tolist() == inter.tolist()
    cnt = b"".join(key + struct.pack("<3I", *row) for row in ((1, 2, 0), (5, 0, 7), (3, 3, 3)))
    inter, mins = both(cnt, 3, 1, COUNT, mins=True)
    assert inter.tolist() == [[3, 2, 2], [2, 2, 1], [2, 1, 2]]
    assert mins.tolist() == [[9, 4, 8], [4, 5, 3], [8, 3, 10]]
    assert "%.6f" % dr.jaccard(inter, 0, 1) == "0.333333"
    assert "%.6f" % dr.braycurtis(mins, 0, 1) == "0.428571"
    # a PA row of a one-word key and 13 bytes is 21 bytes long
    assert dr.row_bytes(1, 100, PA) == 21 and dr.row_bytes(0, 100, BF) == 13 and dr.row_bytes(2, 100, COUNT) == 416


def test_the_two_roads_agree():
    """N 1 ... 130 with every padding bit set; fills 0, 0.02, 0.5 and 1; counts including 2^32 - 1"""
    fills = (0.0, 0.02, 0.5, 1.0)
    for N in range(1, 131):
        fill = fills[N % 4]
        rows = 1 + (N * 7) % 23
        inter, _ = both(dr.make_body(N, rows, N, 1 + N % 4, PA, fill), N, 1 + N % 4, PA)
        assert np.array_equal(inter, inter.T) and int(inter.max(initial=0)) <= rows
        if fill == 1.0:
            assert (inter == rows).all()      # (a padding bit that reached a result would not change this; the next line's would)
        if fill == 0.0:
            assert not inter.any()            # every padding bit is set in the body: none of them is counted
        both(dr.make_body(N + 1000, rows, N, 0, BF, fill), N, 0, BF)
        inter, mins = both(dr.make_body(N + 2000, rows, N, 1 + N % 4, COUNT, fill, maxed=0.3), N, 1 + N % 4, COUNT, mins=True)
        assert np.array_equal(mins, mins.T) and (mins >= inter).all()
        if fill == 1.0 and rows >= 5:
            assert int(mins.max()) > 2 ** 32
    # five rows of 2^32 - 1 in every column: mins pass 2^34
    body = dr.make_body(1, 5, 9, 1, COUNT, 1.0, lo=0xFFFFFFFF, hi=0x100000000)
    inter, mins = both(body, 9, 1, COUNT, mins=True)
    assert (inter == 5).all() and (mins == 5 * 0xFFFFFFFF).all() and int(mins[0, 0]) > 2 ** 34


def test_tables_add_up_over_cuts():
    """the rows of a body cut anywhere: the parts' tables add up to the whole's"""
    N, kw = 67, 2
    body = dr.make_body(3, 200, N, kw, COUNT, 0.3, maxed=0.05)
    rb = dr.row_bytes(kw, N, COUNT)
    whole = dr.dist_expected_np(body, N, kw, COUNT, mins=True)
    parts = [dr.dist_expected_np(body[a * rb:b * rb], N, kw, COUNT, mins=True) for a, b in ((0, 1), (1, 130), (130, 130), (130, 200))]
    assert np.array_equal(sum(p[0] for p in parts), whole[0]) and np.array_equal(sum(p[1] for p in parts), whole[1])


def test_text_format():
    ids = ["D1", "D2", "D3"]
    inter = np.array([[3, 2, 0], [2, 2, 0], [0, 0, 0]], np.uint64)
    mins = np.array([[9, 4, 0], [4, 5, 0], [0, 0, 0]], np.uint64)
    assert dr.format_table(ids, "shared", inter) == "\tD1\tD2\tD3\nD1\t3\t2\t0\nD2\t2\t2\t0\nD3\t0\t0\t0\n"
    # a zero denominator (sample 3 is empty) prints 0.000000
    assert dr.format_table(ids, "jaccard", inter) == ("\tD1\tD2\tD3\nD1\t0.000000\t0.333333\t1.000000\nD2\t0.333333\t0.000000\t1.000000\n"
                                                      "D3\t1.000000\t1.000000\t0.000000\n")
    assert dr.format_table(ids, "braycurtis", inter, mins) == ("\tD1\tD2\tD3\nD1\t0.000000\t0.428571\t1.000000\nD2\t0.428571\t0.000000\t1.000000\n"
                                                               "D3\t1.000000\t1.000000\t0.000000\n")
    big = np.array([[2 ** 40 + 1]], np.uint64)
    assert dr.format_table(["x"], "shared", big) == f"\tx\nx\t{2 ** 40 + 1}\n"


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"#define KMX_VERSION 2\b", hdr)
    declared = set(re.findall(r"\b(kmx_dist_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"DIST_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no DIST_EXPORTS"
    bound = set(re.findall(r'"(kmx_dist_\w+)"', listed.group(1)))
    want = {"kmx_dist_dev", "kmx_dist_host"} | {"kmx_dist_result_" + s for s in
            ("wait", "inter_dev", "mins_dev", "copy_inter", "copy_mins", "kernel_ms", "kernel_parts_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert "kmx_dist_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]      # the opening list of entry points
    assert re.search(r"\bKMX_VERSION = 2\b", src)
    # the binding's structure has the header's fields in the header's order
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_dist_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    struct_src = re.search(r"class KmxDistTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    assert c_fields == ["key_words", "mode", "n_cols", "want_mins", "rows", "n_rows", "inter", "mins"]
    for name in ("KmxDistTask", "DistResult", "DistOutput", "def dist(", "def dist_dev("):
        assert name in src, name


def test_library_exports_the_symbols():
    """the built library has them (and kmx_version is unchanged)"""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert lib.kmx_version() == 2
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    names = re.findall(r'"(kmx_dist_\w+)"', re.search(r"DIST_EXPORTS = \[(.*?)\]", src, re.S).group(1))
    assert len(names) == 11
    for name in names:
        assert hasattr(lib, name), name


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output -------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def refused(*args, word=None):
    r = kmx("dist", *args)
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert word is None or word in r.stderr, (args, r.stderr)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxdist")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in dr.KINDS:
        kw = {"kmer": 1, "hash": 1}[mode.split(":")[0]] if mode != "hash:bf:bin" else 0
        rmode = dr.KINDS[mode][5]
        bodies = [dr.make_body(p, 10 if rmode != BF else 16, 3, kw, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    return dict(dir=d, runs=out, ids=ids, k=k)


def test_driver_refuses_what_is_no_run(runs, tmp_path):
    refused(word="--run")
    refused("--run", tmp_path / "nothing", word="not a kmtricks runtime directory")
    os.makedirs(tmp_path / "empty")
    refused("--run", tmp_path / "empty", word="not a kmtricks runtime directory")
    refused("--run", runs["runs"]["kmer:count:bin"], "--metric", "euclid", word="--metric")
    refused("--run", runs["runs"]["kmer:count:bin"], "--frobnicate")


def test_driver_refuses_modes_it_does_not_read(runs):
    body = dr.make_body(1, 4, 3, 1, COUNT)
    for said in ("hash:bfc:bin", "hash:bft:bin", "kmer:count:text", "kmer:pa:text", "hash:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused("--run", root, word=said)


def test_driver_refuses_braycurtis_without_counts(runs):
    for mode in ("kmer:pa:bin", "hash:pa:bin", "hash:bf:bin"):
        refused("--run", runs["runs"][mode], "--metric", "braycurtis", word="braycurtis")


def test_driver_refuses_gpus_out_of_range(runs):
    for g in (0, 17, 1000):
        refused("--run", runs["runs"]["kmer:pa:bin"], "--gpus", g, word="--gpus")
    refused("--run", runs["runs"]["kmer:pa:bin"], "--gpus", "two", word="--gpus")


@pytest.mark.parametrize("mode", list(dr.KINDS))
def test_driver_refuses_files_that_do_not_fit(runs, mode, tmp_path):
    ext, hdr, magic, cols_at, kw, rmode = dr.KINDS[mode]
    src = runs["runs"][mode]
    f1 = os.path.join("matrices", f"matrix_1.{ext}")

    def variant(name):
        shutil.copytree(src, tmp_path / name)
        return tmp_path / name

    d = variant("cut")           # a body that is no whole number of rows
    with open(d / f1, "r+b") as f:
        f.truncate(os.path.getsize(d / f1) - 1)
    refused("--run", d, word=f"matrix_1.{ext}")
    d = variant("gone")          # a partition without its file
    os.remove(d / f1)
    refused("--run", d, word=f"matrix_1.{ext}")
    d = variant("cols")          # a header of another number of columns than the fof has samples
    with open(d / f1, "r+b") as f:
        f.seek(cols_at); f.write(struct.pack("<I", 4))
    refused("--run", d, word=f"matrix_1.{ext}")
    d = variant("fof")           # a fof of one sample more
    with open(d / "kmtricks.fof", "a") as f:
        f.write("D : /nowhere/D.fasta\n")
    refused("--run", d, word="4 samples")
    d = variant("magic")         # another kind of file under the name
    with open(d / f1, "r+b") as f:
        f.seek(13); f.write(struct.pack("<Q", 0x1234))
    refused("--run", d, word="Invalid file format")
    if mode.startswith("kmer:"):
        d = variant("k")         # a header of another k than options.txt names
        with open(d / f1, "r+b") as f:
            f.seek(21); f.write(struct.pack("<I", 33))
        refused("--run", d, word="k = 33")
    if mode == "hash:bf:bin":
        d = variant("window")    # a window that disagrees with hash.info
        with open(d / f1, "r+b") as f:
            f.seek(33); f.write(struct.pack("<Q", 17))
        refused("--run", d, word="hash.info")
