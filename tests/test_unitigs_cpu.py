"""kmx_unitigs_* / kmx_groupsum_* / `kmx unitigs` without a device: the header's worked examples as literals on both roads of
tests/unitig_ref.py, the two roads on every case the GPU test walks, what that list of cases covers, the ABI, the driver's refusals (every
one comes before kmx_create), its --kmers parser and its file formats."""
import ctypes, os, re, subprocess
import numpy as np
import pytest

import dist_ref as dr
import unitig_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = ur.MODE_COUNT, ur.MODE_PA
USAGE = ("kmx unitigs --run <run dir made with --mode kmer:count:bin or kmer:pa:bin, plain or --cpr> [--kmers FILE] [--output FILE] "
         "[--table FILE [--value mean|frac|sum|present]] [--samples FILE] [--min-abund INT] [--batch-mb INT] [--gpus INT] [-v]")
ROADS = (ur.unitigs_links, ur.unitigs_walk)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_worked_examples():
    """the examples of include/kmx.h, section unitigs, as literals, on both roads"""
    keys = [ur.enc(s) for s in ("ATTGC", "CAATG", "CAGGA", "CCTGC", "CTGCA", "TTGCA", "TGCAC")]
    assert keys == [173, 267, 316, 365, 436, 692, 721]
    for road in ROADS:
        r = road(keys, 5)
        assert r.U == 3 and r.seqs == ["CATTGCA", "TCCTGCA", "TGCAC"]
        assert r.unitig == [0, 0, 1, 1, 1, 0, 2] and r.pos == [1, 0, 0, 1, 2, 2, 0] and r.ori == [0, 1, 1, 0, 0, 0, 0]
        assert r.start == [1, 2, 6] and r.len == [3, 3, 1] and r.circ == [0, 0, 0] and r.seq_off(5) == [0, 7, 14, 19]
    keys = [ur.enc(s) for s in ("ACCTG", "AGGTC", "CCTGA", "CTGAC", "TGACC")]
    for road in ROADS:
        r = road(keys, 5)
        assert r.U == 1 and r.seqs == ["ACCTGACCT"] and r.pos == [0, 4, 1, 2, 3] and r.ori == [0, 1, 0, 0, 0] and r.circ == [1] and r.len == [5]
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for text in ("(173, 267, 316, 365, 436, 692, 721)", "CATTGCA, TCCTGCA, TGCAC", "unitig = (0,0,1,1,1,0,2), pos = (1,0,0,1,2,2,0), ori = (0,1,1,0,0,0,0)",
                 "start = (1,2,6)", "len = (3,3,1)", "seq ACCTGACCT, pos = (0,4,1,2,3), ori = (0,1,0,0,0), circ = (1)"):
        assert text in hdr, text


def test_groupsum_example_and_the_two_roads():
    """the example of section groupsum as literals; numpy against plain loops over modes, lists, windows and min_abund"""
    counts = np.array([[1, 0, 2], [0, 0, 5], [3, 0, 1], [4, 4, 4]], np.uint32)
    for road in (ur.groupsum_np, ur.groupsum_loops):
        size, present, sums = road(counts, [7, 8, 7, 0xFFFFFFFF], None, 1, 7, 2, COUNT, True)
        assert size.tolist() == [2, 1] and present.tolist() == [[2, 0, 2], [0, 0, 1]] and sums.tolist() == [[4, 0, 3], [0, 0, 5]]
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert "size = (2, 1), present = ((2,0,2), (0,0,1)), sums = ((4,0,3), (0,0,5))" in hdr
    rng = np.random.default_rng(3)
    for mode in (COUNT, PA):
        for N, rows in ((1, 40), (9, 200), (70, 120)):
            _, counts = ur.make_body(rng, rows, N, 1, mode)
            g = rng.integers(0, 12, rows).astype(np.uint32)
            g[::9] = 0xFFFFFFFF
            for cols, a, g0, G in ((None, 1, 0, 12), (rng.permutation(N)[:max(1, N // 2)], 2 if mode == COUNT else 1, 3, 5), (None, 1, 11, 40)):
                x, y = ur.groupsum_np(counts, g, cols, a, g0, G, mode, mode == COUNT), ur.groupsum_loops(counts, g, cols, a, g0, G, mode, mode == COUNT)
                assert all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(x, y))


def test_the_two_roads_agree_on_the_gpu_cases():
    """sequences, circular flags and unitig / pos / ori of every case tests/test_unitigs_gpu.py walks"""
    for name, k, keys in ur.cases():
        assert len(set(keys)) == len(keys) and all(x == ur.canon_int(x, k) for x in keys), name
        a, b = ur.expected(name), ur.unitigs_walk(keys, k)
        assert a.same(b), name
        assert sum(a.len) == len(keys) and [a.unitig[s] for s in a.start] == list(range(a.U)) and a.start == sorted(a.start), name


def test_two_extensions_of_one_side_are_never_one_node():
    """x[1:] + c == revcomp(x[1:] + d) forces c == d (then the extension is its own reverse complement and one string): the two present
    extensions of a side are always two nodes, so the degree counts nodes as well as strings.  Every z of 3 ... 6 bases, every (c, d)"""
    for m in range(3, 7):
        for z in range(4 ** m):
            for c in range(4):
                for d in range(4):
                    if c != d:
                        assert (z << 2 | c) != ur.rc_int(z << 2 | d, m + 1)


def test_sweep_covers_every_axis():
    """from road A: the list really contains what the GPU test is meant to meet"""
    cases = ur.cases()
    by = {name: (k, keys) for name, k, keys in cases}
    seen = dict(pal_kw=set(), self_loop=False, hairpin=False, both_sides_one_node=False, deg=set(), high_end=False, cyc_index_not_key=False,
                cyc_reversed=False, shuffled=False, sorted=False)
    for name, k, keys in cases:
        n = len(keys)
        index = {x: i for i, x in enumerate(keys)}
        r = ur.expected(name)
        _, deg = ur.links_of(keys, k)
        seen["deg"] |= set(deg)
        if n > 2:
            seen["sorted" if keys == sorted(keys) else "shuffled"] = True
        for v in range(n):
            ext = [ur.extensions(keys, index, k, v, s) for s in (0, 1)]
            if keys[v] == ur.rc_int(keys[v], k) and k % 2 == 0 and any(u != v for e in ext for u, _, _ in e):
                seen["pal_kw"].add(ur.key_words_of(k))
            for s in (0, 1):
                for u, t, _ in ext[s]:
                    if u == v and t != s:
                        seen["self_loop"] = True      # leaves through s, comes back through the other side
                    if u == v and t == s:
                        seen["hairpin"] = True        # comes back through the side it left
            if {u for u, _, _ in ext[0]} & {u for u, _, _ in ext[1]} - {v}:
                seen["both_sides_one_node"] = True
        for u in range(r.U):
            nodes = [v for v in range(n) if r.unitig[v] == u] if r.U < 50 else None
            if nodes is None:
                continue
            if r.circ[u]:
                m = min(nodes)
                seen["cyc_index_not_key"] |= r.start[u] != m
                seen["cyc_reversed"] |= r.ori[m] == 1      # the owner leaves m through side 1: m read forward; the unitig reads it reversed
            elif r.len[u] > 1:
                last = next(v for v in nodes if r.pos[v] == r.len[u] - 1)
                seen["high_end"] |= r.start[u] > last
    assert seen["pal_kw"] == {1, 2, 3, 4}, seen
    assert seen["self_loop"] and seen["hairpin"] and seen["both_sides_one_node"], seen
    assert seen["deg"] == {0, 1, 2, 3, 4}, seen
    assert seen["high_end"] and seen["cyc_index_not_key"] and seen["cyc_reversed"] and seen["shuffled"] and seen["sorted"], seen
    for n in ur.PATH_L:      # one path of L = n: the round count's edges (R = bit_length(n - 1) + 1)
        k, keys = by[f"path_{n}"]
        r = ur.expected(f"path_{n}")
        assert k == 31 and len(keys) == n and r.U == 1 and r.len == [n] and r.circ == [0]
    assert set(ur.PATH_L) == {1, 2, 3, 4, 5, 8, 9, 16, 17, 1023, 1024, 1025, 4097}
    for n in ur.CYCLE_L:
        k, keys = by[f"cycle_{n}"]
        r = ur.expected(f"cycle_{n}")
        assert k == 31 and len(keys) == n and r.U == 1 and r.len == [n] and r.circ == [1]
    assert set(ur.CYCLE_L) == {2, 3, 4, 5, 64, 65, 1024, 1025}
    assert {8, 12, 31, 32, 33, 63, 64, 65, 96, 97, 126, 127} <= {k for _, k, _ in cases}
    assert any(sum(ur.expected(name).circ) > 1 for name, _, _ in cases)      # several cycles in one call


# ---- header, binding, sources --------------------------------------------------------------------------------------------------------
UNITIGS = {"kmx_unitigs_dev", "kmx_unitigs_host"} | {"kmx_unitigs_result_" + s for s in (
    "wait", "n_unitigs", "unitig_dev", "copy_unitig", "copy_pos", "copy_ori", "copy_start", "copy_len", "copy_circ", "copy_seq_off", "seq_bytes", "copy_seqs",
    "kernel_ms", "kernel_parts_ms", "algo_bytes", "free")}
GROUPSUM = {"kmx_groupsum_dev", "kmx_groupsum_host"} | {"kmx_groupsum_result_" + s for s in (
    "wait", "present_dev", "sums_dev", "size_dev", "copy_present", "copy_sums", "copy_size", "kernel_ms", "algo_bytes", "free")}


def c_fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr, re.S).group(1), flags=re.S)
    return [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert set(re.findall(r"\b(kmx_unitigs_\w+)\s*\(", hdr)) == UNITIGS
    assert set(re.findall(r"\b(kmx_groupsum_\w+)\s*\(", hdr)) == GROUPSUM
    from kmtricks_amd import lib
    assert set(lib.UNITIGS_EXPORTS) == UNITIGS and set(lib.GROUPSUM_EXPORTS) == GROUPSUM
    assert "kmx_unitigs_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")] and "kmx_groupsum_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]
    assert "/* ---------------------------------------------------------------- unitigs */" in hdr
    assert "/* --------------------------------------------------------------- groupsum */" in hdr
    assert c_fields(hdr, "kmx_unitigs_task") == [f[0] for f in lib.KmxUnitigsTask._fields_]
    assert c_fields(hdr, "kmx_groupsum_task") == [f[0] for f in lib.KmxGroupsumTask._fields_]
    assert "109 bytes a node at the most" in hdr and "8 * key_words + 26 bytes" in hdr      # scratch and result per node are stated


def test_library_and_binding_structures():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    for name in sorted(UNITIGS | GROUPSUM):
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxUnitigsTask) == 32 and lib.KmxUnitigsTask.kmer_size.offset == 16 and lib.KmxUnitigsTask.flags.offset == 24
    assert ctypes.sizeof(lib.KmxGroupsumTask) == 88 and lib.KmxGroupsumTask.groups.offset == 40 and lib.KmxGroupsumTask.g0.offset == 56
    assert lib.KmxGroupsumTask.present.offset == 64 and lib.KmxGroupsumTask.size.offset == 80 and lib.GROUPSUM_SUMS == 1
    csrc = os.path.join(ROOT, "kmtricks_amd", "csrc")
    src = open(os.path.join(csrc, "unitigs.hip")).read()
    assert "static_assert(sizeof(kmx_unitigs_task) == 32" in src
    for read in ('kmx_env_cus("KMX_UNITIG_CUS", ctx)', 'kmx_env_grid("KMX_UNITIG_GRID", planned)', 'kmx_env_int("KMX_UNITIG_HASH_BITS")'):
        assert read in src, read
    gsrc = open(os.path.join(csrc, "groupsum.hip")).read()
    assert "static_assert(sizeof(kmx_groupsum_task) == 88" in gsrc and "mat_call(" in gsrc and "mat_row_plan(" in gsrc
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "unitigs.hip" in mk and "groupsum.hip" in mk
    assert "kmx_unitigs.cpp" in open(os.path.join(ROOT, "kmtricks_amd", "host", "Makefile")).read()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def test_usage_is_pinned():
    r = kmx("unitigs")
    assert r.returncode == 1 and r.stdout == "" and "usage: " + USAGE in r.stderr
    assert "reads the partitions again" in r.stderr
    assert USAGE.replace("|", "\\|") in open(os.path.join(ROOT, "README.md")).read()      # (a table cell escapes the bar)


def key_body(keys, k, n_cols, mode, seed):
    """a matrix body whose rows carry the given keys (ascending)"""
    rng = np.random.default_rng(seed)
    kw = ur.key_words_of(k)
    body, counts = ur.make_body(rng, len(keys), n_cols, kw, mode)
    rb = len(body) // max(len(keys), 1)
    a = np.frombuffer(body, np.uint8).reshape(len(keys), rb).copy()
    a[:, :8 * kw] = ur.keys_to_words(sorted(keys), k).view(np.uint8).reshape(len(keys), 8 * kw)
    return a.tobytes()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import random
    d = tmp_path_factory.mktemp("kmxunitigs")
    ids, k = ["A", "B", "C"], 31
    rng = random.Random(1)
    parts = [ur.kmers_of(ur.rand_seq(rng, 60), k) for _ in range(2)]
    out = {}
    for mode in ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin"):
        rmode = dr.KINDS[mode][5]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, [key_body(p, k, 3, rmode, i) for i, p in enumerate(parts)], window=16)
    return dict(dir=d, runs=out, ids=ids, k=k, parts=parts)


def refused(tmp_path, *args, text=None, outputs=True):
    outs = [tmp_path / "out.fa", tmp_path / "table.tsv"]
    r = kmx("unitigs", *(["--output", outs[0], "--table", outs[1]] if outputs else []), *args)
    assert r.returncode == 1 and r.stderr.startswith("[error] ") and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert text is None or r.stderr.startswith("[error] " + text), (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert not any(os.path.exists(p) for p in outs), "a refusal wrote a file"


def test_driver_refuses_bad_options(runs, tmp_path):
    run = runs["runs"]["kmer:count:bin"]
    refused(tmp_path, "--run", tmp_path / "nothing", text=f"{tmp_path / 'nothing'} is not a kmtricks runtime directory.\n")
    refused(tmp_path, "--run", run, "--frobnicate", text="unknown option --frobnicate\nusage: " + USAGE)
    refused(tmp_path, text="--run is required\nusage: " + USAGE)
    refused(tmp_path, "--run", run, text="one of --output and --table is required\nusage: " + USAGE, outputs=False)
    refused(tmp_path, "--run", run, "--output", tmp_path / "o.fa", "--value", "sum", text="--value needs --table\n", outputs=False)
    refused(tmp_path, "--run", run, "--value", "median", text="--value must be mean, frac, sum or present\n")
    refused(tmp_path, "--run", run, "--min-abund", 0, text="--min-abund must be at least 1\n")
    refused(tmp_path, "--run", run, "--min-abund", "-1", text="bad number for --min-abund: -1\n")
    refused(tmp_path, "--run", run, "--min-abund", 2 ** 32, text="--min-abund does not fit 32 bits\n")
    for g in (0, 17):
        refused(tmp_path, "--run", run, "--gpus", g, text="--gpus must be in [1, 16]\n")
    refused(tmp_path, "--run", run, "--kmers", text="missing value for --kmers\n")
    refused(tmp_path, "--run", run, "--kmers", tmp_path / "none.tsv", text=f"Unable to read at {tmp_path / 'none.tsv'}\n")
    refused(tmp_path, "--run", run, "--samples", tmp_path / "none.txt", text=f"Unable to read at {tmp_path / 'none.txt'}\n")
    with open(tmp_path / "s.txt", "w") as f:
        f.write("A\nZ\n")
    refused(tmp_path, "--run", run, "--samples", tmp_path / "s.txt", text=f"{tmp_path / 's.txt'} line 2: sample Z is not in the run's kmtricks.fof\n")
    pa = runs["runs"]["kmer:pa:bin"]
    refused(tmp_path, "--run", pa, "--min-abund", 2, text="--min-abund above 1 needs counts")
    for v in ("sum", "mean"):
        refused(tmp_path, "--run", pa, "--value", v, text=f"--value {v} needs counts")


def test_driver_refuses_runs_whose_keys_are_no_kmers(runs, tmp_path):
    for mode in ("hash:count:bin", "hash:pa:bin"):
        refused(tmp_path, "--run", runs["runs"][mode], text="kmx unitigs needs a run made with --mode kmer:count:bin or kmer:pa:bin (the keys of hash and Bloom filter runs are not k-mers)")
    body = key_body(runs["parts"][0], 31, 3, COUNT, 0)
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused(tmp_path, "--run", root, text="kmx unitigs needs a run made with")


@pytest.mark.parametrize("text,word", [("ACGT\n", "line 1: a k-mer of 4 characters, the run's k is 31"), ("#c\n" + "A" * 32 + "\tx\n", "line 2: a k-mer of 32 characters"),
                                       ("A" * 30 + "N\t1\n", "line 1: malformed k-mer"), ("A" * 31 + "\n\n" + "A" * 15 + "-" + "C" * 15 + "\n", "line 3: malformed k-mer"),
                                       ("A" * 31 + " 3\n", "line 1: a k-mer of 33 characters")])
def test_driver_refuses_malformed_kmer_lists(runs, tmp_path, text, word):
    with open(tmp_path / "k.tsv", "w") as f:
        f.write(text)
    refused(tmp_path, "--run", runs["runs"]["kmer:count:bin"], "--kmers", tmp_path / "k.tsv", text=f"{tmp_path / 'k.tsv'} {word}")
    with pytest.raises(ValueError):
        ur.parse_kmers(text, 31)


def test_kmers_parser_restated():
    """the first tab-separated field, # lines and empty lines skipped, either strand and either case, CRLF"""
    s = "ACGTTGCAAGGCTTAACCGGTTACGATCGAT"
    text = f"# kmx diff\nkmer_is_not_here\n".replace("kmer_is_not_here", s) + f"{ur.rc_str(s).lower()}\tcase\t0.1\r\n\n{'C' * 31}\tx\n"
    got = ur.parse_kmers(text, 31)
    assert got == {ur.canon_int(ur.enc(s), 31), ur.canon_int(ur.enc("C" * 31), 31)} and len(got) == 2


def test_file_formats_restated():
    """FASTA headers and the four table values on a result made by hand"""
    r = ur.Unitigs([0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 2], [2, 1], [1, 0], ["ACGTAC", "TTTTT"])
    assert ur.fasta_text(r, 5) == ">0 LN:i:6 KM:i:2 CL:Z:circular\nACGTAC\n>1 LN:i:5 KM:i:1\nTTTTT\n"
    size, present, sums = np.array([3, 1]), np.array([[2, 0], [1, 1]]), np.array([[7, 0], [2 ** 33, 5]])
    assert ur.table_text(["A", "B"], size, present, sums, "sum") == "unitig\tkmers\tA\tB\n0\t3\t7\t0\n1\t1\t8589934592\t5\n"
    assert ur.table_text(["A", "B"], size, present, sums, "present") == "unitig\tkmers\tA\tB\n0\t3\t2\t0\n1\t1\t1\t1\n"
    assert ur.table_text(["A", "B"], size, present, sums, "mean") == "unitig\tkmers\tA\tB\n0\t3\t2.33\t0.00\n1\t1\t8589934592.00\t5.00\n"
    assert ur.table_text(["A", "B"], size, present, sums, "frac") == "unitig\tkmers\tA\tB\n0\t3\t0.67\t0.00\n1\t1\t1.00\t1.00\n"
