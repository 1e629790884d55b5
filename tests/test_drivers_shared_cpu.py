"""CPU-only: the refusals that the run-reading drivers of `kmx` share (kmtricks_amd/host/kmx_driver.hpp) and that no other test reaches,
one table for all of them: tool -> the arguments it cannot do without -> the modes it reads -> how it words them.  Each case is one
`[error]` line before any device is asked for, on run directories written by hand (dist_ref.write_run: 3 samples, k = 31, 2
partitions of 10 rows)."""
import os
import shutil
import struct
import subprocess

import pytest

import dist_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
KMER = ("kmer:count:bin", "kmer:pa:bin")
FOUR = KMER + ("hash:count:bin", "hash:pa:bin")
FOUR_WORDS = "kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin"
# tool -> (extra arguments; {d} is a directory with the files `groups` and `pheno`, {out} a path that is not there), modes, wording)
TOOLS = {
    "select": (("--output", "{out}"), FOUR, FOUR_WORDS),
    "dist": ((), FOUR + ("hash:bf:bin",), "kmer:count:bin, kmer:pa:bin, hash:count:bin, hash:pa:bin or hash:bf:bin"),
    "diff": (("--groups", "{d}/groups"), FOUR, FOUR_WORDS),
    "pan": ((), FOUR, FOUR_WORDS),
    "colors": ((), FOUR, FOUR_WORDS),
    "pca": ((), FOUR, FOUR_WORDS),
    "assoc": (("--pheno", "{d}/pheno"), FOUR, FOUR_WORDS),
    "unitigs": (("--output", "{out}"), KMER, "kmer:count:bin or kmer:pa:bin (the keys of hash and Bloom filter runs are not k-mers)"),
}
CASES = [(tool, mode) for tool, (_, modes, _) in TOOLS.items() for mode in modes]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxshared")
    ids, out = ["A", "B", "C"], {}
    for mode in TOOLS["dist"][1]:
        kw, rmode = dr.KINDS[mode][4], dr.KINDS[mode][5]
        rows = 16 if mode == "hash:bf:bin" else 10      # (a Bloom matrix has a window of rows)
        bodies = [dr.make_body(p, rows, 3, 1 if kw is None else kw, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, 31, ids, bodies, window=16)
    with open(d / "groups", "w") as f:
        f.write("A control\nB case\nC case\n")
    with open(d / "pheno", "w") as f:
        f.write("A 0.5\nB 1.5\nC -2\n")
    return dict(dir=d, runs=out)


def refused(runs, tmp_path, tool, run, text, *more):
    """`kmx tool --run run` and the tool's own arguments: the one line `text`, status 1, nothing on standard output, nothing written"""
    out = tmp_path / "out"
    extra = [a.format(d=runs["dir"], out=out) for a in TOOLS[tool][0]]
    r = subprocess.run([KMX, tool, "--run", str(run)] + extra + [str(a) for a in more], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "[error] " + text + "\n"), (tool, run, r.returncode, r.stdout[:200], r.stderr)
    assert not os.path.exists(out), "a refusal wrote a file"


def variant(runs, tmp_path, mode, name):
    shutil.copytree(runs["runs"][mode], tmp_path / name)
    return tmp_path / name


def set_option(d, old, new):
    line = open(d / "options.txt").read()
    assert old in line
    with open(d / "options.txt", "w") as f:
        f.write(line.replace(old, new))


@pytest.mark.parametrize("tool,mode", CASES)
def test_refusals_of_the_run_that_no_tool_was_tested_for(runs, tmp_path, tool, mode):
    ext, hdr, magic, cols_at, kw, rmode = dr.KINDS[mode]
    f0, f1 = (os.path.join("matrices", f"matrix_{p}.{ext}") for p in (0, 1))
    d = variant(runs, tmp_path, mode, "nok")           # options.txt without a kmer_size
    set_option(d, " kmer_size=31,", "")
    refused(runs, tmp_path, tool, d, f"{d}/options.txt names no kmer_size")
    for k in (7, 128):                                  # ... with one outside what a key holds
        d = variant(runs, tmp_path, mode, f"k{k}")
        set_option(d, "kmer_size=31", f"kmer_size={k}")
        refused(runs, tmp_path, tool, d, "the run's options.txt names a k-mer size outside [8, 127]")
    if mode in KMER:                                    # ... with another than the matrices were made with
        d = variant(runs, tmp_path, mode, "k33")
        set_option(d, "kmer_size=31", "kmer_size=33")
        refused(runs, tmp_path, tool, d, f"{d / f0} was made with k = 31 in 1 words, the run's options.txt says 33")
    if mode == "hash:count:bin":                        # counts of another width
        d = variant(runs, tmp_path, mode, "c2")
        with open(d / f1, "r+b") as f:
            f.seek(21); f.write(struct.pack("<I", 2))
        refused(runs, tmp_path, tool, d, f"{d / f1} has counts of 2 bytes: kmx {tool} reads 4-byte counts")
    # a partition count that is none (dist, which reads a Bloom run's window beside it, words the two as one)
    none = "the run's partition count and window do not fit together" if tool == "dist" else "the run's partition count is outside [1, 65535]"
    for P in (0,) if mode in KMER else (0, 65536):
        d = variant(runs, tmp_path, mode, f"p{P}")
        if mode in KMER:
            raw = open(d / "repartition_gatb" / "repartition.minimRepart", "rb").read()
            with open(d / "repartition_gatb" / "repartition.minimRepart", "wb") as f:
                f.write(struct.pack("<H", P) + raw[2:])
        else:
            with open(d / "hash.info", "r+b") as f:
                f.seek(8); f.write(struct.pack("<Q", P))
        refused(runs, tmp_path, tool, d, none)


@pytest.mark.parametrize("tool", ["assoc", "unitigs"])
def test_a_mode_the_tool_does_not_read_is_named_in_full(runs, tmp_path, tool):
    said = "hash:bft:bin"
    body = dr.make_body(1, 4, 3, 1, dr.MODE_COUNT)
    root = dr.write_run(tmp_path / "said", "kmer:count:bin", 31, ["A", "B", "C"], [body], options_mode=said)
    refused(runs, tmp_path, tool, root, f"kmx {tool} needs a run made with --mode {TOOLS[tool][2]}; {root} was made with {said}")


@pytest.mark.parametrize("tool,mode", [c for c in CASES if c[0] in ("assoc", "unitigs")])
def test_files_that_do_not_fit(runs, tmp_path, tool, mode):
    """what select, dist, diff, pan, colors and pca are tested for in their own files"""
    ext, hdr, magic, cols_at, kw, rmode = dr.KINDS[mode]
    f0, f1 = (os.path.join("matrices", f"matrix_{p}.{ext}") for p in (0, 1))
    stride = dr.row_bytes(1, 3, rmode)
    d = variant(runs, tmp_path, mode, "cut")           # a truncated body: no whole number of rows
    with open(d / f1, "r+b") as f:
        f.truncate(os.path.getsize(d / f1) - 1)
    refused(runs, tmp_path, tool, d, f"truncated matrix (its body is no whole number of rows of {stride} bytes): {d / f1}")
    d = variant(runs, tmp_path, mode, "gone")          # a missing matrix
    os.remove(d / f1)
    refused(runs, tmp_path, tool, d, f"Unable to read at {d / f1}")
    d = variant(runs, tmp_path, mode, "cols")          # a header of another number of columns than the fof has samples
    with open(d / f1, "r+b") as f:
        f.seek(cols_at); f.write(struct.pack("<I", 4))
    refused(runs, tmp_path, tool, d, f"{d / f1} has rows of 4 columns, the run's kmtricks.fof has 3 samples")
    d = variant(runs, tmp_path, mode, "magic")         # another kind of file under the name
    with open(d / f1, "r+b") as f:
        f.seek(13); f.write(struct.pack("<Q", 0x1234))
    refused(runs, tmp_path, tool, d, f"Invalid file format: {d / f1}")
    d = variant(runs, tmp_path, mode, "nofof")         # a fof with a sample more than the matrices have columns
    with open(d / "kmtricks.fof", "a") as f:
        f.write("D : /nowhere/D.fasta\n")
    refused(runs, tmp_path, tool, d, f"{d / f0} has rows of 3 columns, the run's kmtricks.fof has 4 samples")
    d = variant(runs, tmp_path, mode, "noopt")
    os.remove(d / "options.txt")
    refused(runs, tmp_path, tool, d, f"Unable to read at {d}/options.txt")
    d = variant(runs, tmp_path, mode, "noparts")       # the partition count's file
    name = "repartition_gatb/repartition.minimRepart" if mode in KMER else "hash.info"
    os.remove(d / name)
    refused(runs, tmp_path, tool, d, f"Unable to read at {d}/{name}")


@pytest.mark.parametrize("option,value", [("--batch-mb", "-1"), ("--gpus", "-1")])
def test_dist_reads_numbers_as_the_other_tools_do(runs, tmp_path, option, value):
    """a leading `-` is no number: `--batch-mb -1` used to wrap to a budget of 2^64 - 1 MiB and go on to the device"""
    refused(runs, tmp_path, "dist", runs["runs"]["kmer:count:bin"], f"bad number for {option}: {value}", option, value)
