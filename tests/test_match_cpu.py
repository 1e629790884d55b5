"""kmx_kset_* / kmx_match_* / `kmx match` without a device: the header's worked example as literals on both roads of tests/match_ref.py,
the two roads on every case the GPU test walks, what that list of cases covers, the ABI, the driver's usage and refusals (every one comes
before kmx_create), and its parsers and file formats restated."""
import ctypes, os, re, subprocess
import numpy as np
import pytest

import dist_ref as dr
import match_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
USAGE = ("kmx match (--kmers FILE | --seqs FILE --kmer-size K | --run RUN) --reads FILE [--reads FILE ...] [--output FILE] [--extract FILE] "
         "[--min-hits INT] [--min-frac F] [--min-cover F] [--invert] [--kmer-counts FILE] [--positions FILE] [--batch-mb INT] [--gpus INT] [-v]")
ROADS = (mr.match_strings, mr.match_numpy)
NONE = mr.NONE


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_worked_example():
    """the example of include/kmx.h, section match, as literals, on both roads"""
    keys = [mr.enc(s) for s in ("TTGCA", "ATTGC", "TTGCA", "TGCAC")]
    assert keys == [692, 173, 692, 721] and all(x == mr.canon_of(mr.dec(x, 5)) for x in keys)
    reads = ["CATTGCAC", "ttgcaNtgcaat", "ACGT", "GGGGGGG", "TGCAC"]
    for road in ROADS:
        r = road(keys, 5, reads)
        assert r.key_ids == [0, 1, 0, 3] and r.n_distinct == 3
        assert r.recs == [(4, 3, 3, 7, 1, 3), (3, 3, 1, 11, 0, 7), (0, 0, 0, 0, NONE, NONE), (3, 0, 0, 0, NONE, NONE), (1, 1, 1, 5, 0, 0)]
        assert r.occ == [3, 2, 0, 2]
        assert {p: j for p, j in enumerate(r.ids) if j != NONE} == {1: 1, 2: 0, 3: 3, 8: 0, 14: 0, 15: 1, 31: 3} and len(r.ids) == 36
        assert (r.total_kmers, r.total_hits) == (11, 7)
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for text in ("keys (TTGCA, ATTGC, TTGCA, TGCAC) = (692, 173,", "ids = (0, 1, 0, 3), n_distinct = 3", "(CATTGCAC, ttgcaNtgcaat, ACGT, GGGGGGG, TGCAC)",
                 "(4,3,3,7,1,3), (3,3,1,11,0,7), (0,0,0,0,-,-), (3,0,0,0,-,-), (1,1,1,5,0,0)", "occ = (3, 2, 0, 2)",
                 "1 -> 1, 2 -> 0, 3 -> 3, 8 -> 0, 14 -> 0, 15 -> 1, 31 -> 3"):
        assert text in hdr, text


def test_the_two_roads_agree_on_the_gpu_cases():
    """every record, id and occurrence count of every case tests/test_match_gpu.py walks; the keys are canonical; the sizes stay small"""
    for name, k, keys, reads in mr.cases():
        assert all(x == mr.canon_of(mr.dec(x, k)) for x in keys), name
        assert sum(len(r) for r in reads) <= 300000 and len(keys) <= 100000, name
        a, b = mr.expected(name), mr.match_numpy(keys, k, reads)
        assert a.same(b), name
        assert len(a.ids) == sum(len(r) for r in reads) and sum(a.occ) == a.total_hits == sum(1 for j in a.ids if j != NONE), name
        assert all(a.occ[v] == 0 for v, j in enumerate(a.key_ids) if j != v), name      # only ids are ever counted


def test_sweep_covers_every_axis():
    """from road A: the list really contains what the GPU test is meant to meet"""
    cases = mr.cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    by = {c[0]: c for c in cases}
    # key_words and the top-word mask: every k, and a key that differs from a read's k-mer in one bit of each word
    assert set(mr.K_SWEEP) == {8, 12, 31, 32, 33, 63, 64, 65, 96, 97, 126, 127}
    for k in mr.K_SWEEP:
        _, _, keys, reads = by[f"words_k{k}"]
        own = set(mr.kmers_of(reads, k))
        words = set()
        for x in keys:
            for y in own:
                d = x ^ y
                if d and d & (d - 1) == 0:
                    words.add((d.bit_length() - 1) // 64)
        assert words == set(range(mr.key_words_of(k))), (k, words)
        r = mr.expected(f"words_k{k}")
        assert 0 < r.total_hits < r.total_kmers and any(0 < rec[2] < rec[1] for rec in r.recs), k
    # tiles
    for k in (8, 31):
        _, _, keys, reads = by[f"tiles_k{k}"]
        lens = [len(r) for r in reads]
        assert {k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257} <= set(lens) and lens.count(0) >= 13
        assert sum(lens) % 64 != 0 and lens[-1] > 0      # the last read ends at n_bases, the tile reads past it
        assert any("N" in r for r in reads) and any("n" in r for r in reads) and any(r and r == r.lower() for r in reads)
        r = mr.expected(f"tiles_k{k}")
        assert r.recs[0][0] == 0 and r.recs[2][0] == 1 and r.recs[4][0] == 2      # k - 1, k, k + 1 bases
        bad = next(q for q, s in enumerate(reads) if "N" in s)
        assert r.recs[bad][0] == len(reads[bad]) - k + 1 - 2 * k      # two invalid bases, k positions lost to each
    _, _, _, reads = by["bounds_k8"]
    starts = np.cumsum([0] + [len(r) for r in reads])
    assert [int(s) % 64 for s in starts[1:4]] == [0, 1, 63] and int(starts[-1]) % 64 != 0
    assert by["no_reads"][3] == [] and by["no_reads"][2] and all(r == "" for r in by["empty_reads_only"][3])
    assert max(len(r) for r in by["long_read_k31"][3]) == 200000 and mr.expected("long_read_k31").recs[3][1] >= 3980
    assert len(by["many_reads_k12"][3]) == 5000 and all(len(r) == 30 for r in by["many_reads_k12"][3])
    # cover
    for k in (8, 127):
        for p in mr.COVER_POS:
            rec = mr.expected(f"cover_k{k}_p{p}").recs[0]
            assert rec[1:] == (1, rec[2], k, p, p), (k, p)
        assert set(mr.COVER_POS) == {0, 63, 64, 127, 128}
        for gap, cov in ((-1, 2 * k - 1), (0, 2 * k), (1, 2 * k)):
            rec = mr.expected(f"cover_k{k}_gap{gap}").recs[1]
            assert (rec[1], rec[3], rec[4], rec[5]) == (2, cov, 60, 60 + k + gap), (k, gap)
        r = mr.expected(f"cover_k{k}_all")
        assert all(rec[0] == rec[1] and rec[3] == len(s) for rec, s in zip(r.recs, by[f"cover_k{k}_all"][3]))
    for k in (8, 31):
        _, _, _, reads = by[f"cover_k{k}_last_base"]
        r = mr.expected(f"cover_k{k}_last_base")
        assert r.recs[0][1:] == (1, r.recs[0][2], k, 40 - k, 40 - k) and r.recs[1][1] == 0 and r.recs[1][3] == 0 and len(reads[0]) % 64 != 0
    # the set
    assert set(mr.SET_N) == {0, 1, 2, 255, 256, 257, 4097}
    for n in mr.SET_N:
        assert len(by[f"set_n{n}"][2]) == n == mr.expected(f"set_n{n}").n_distinct
    assert mr.expected("set_n0").total_hits == 0 and mr.expected("set_n0").total_kmers > 0
    _, _, keys, _ = by["dups_k31"]
    copies = sorted(keys.count(x) for x in set(keys))
    r = mr.expected("dups_k31")
    assert copies[0] == 1 and copies[-1] == 50 and r.n_distinct == 60 < len(keys)
    assert any(j != v for v, j in enumerate(r.key_ids)) and any(r.occ[j] > 0 for v, j in enumerate(r.key_ids) if j != v)      # a duplicate whose id is hit
    assert keys != sorted(keys)
    assert r.recs[1][1] > 0 and r.recs[1][2] < r.recs[1][1]      # the reverse strand of the source: hits that are not forward
    assert len(by["n300_k31"][2]) == 300 == len(by["n300_k64"][2])
    assert {mr.key_words_of(k) for k in mr.PAL_K} == {1, 2, 3, 4} and all(k % 2 == 0 for k in mr.PAL_K)
    for k in mr.PAL_K:
        _, _, keys, reads = by[f"palindrome_k{k}"]
        r = mr.expected(f"palindrome_k{k}")
        assert keys[0] == mr.enc(mr.rc_str(mr.dec(keys[0], k))) and r.occ[0] == 2 and r.recs[1] == (1, 1, 1, k, 0, 0)      # a palindrome counts as forward
    r = mr.expected("poly_a_k31")
    assert r.occ == [mr.POLY_HITS + 470, 0] and r.recs[0][:3] == (mr.POLY_HITS,) * 3 and r.recs[2][:3] == (470, 470, 0) and mr.POLY_HITS == 10 ** 5


# ---- header, binding, sources --------------------------------------------------------------------------------------------------------
KSET = {"kmx_kset_" + s for s in ("dev", "host", "wait", "n", "n_distinct", "kmer_size", "copy_ids", "kernel_ms", "free")}
MATCH = {"kmx_match_dev", "kmx_match_host"} | {"kmx_match_result_" + s for s in (
    "wait", "n_seqs", "n_bases", "copy_recs", "copy_ids", "occ_dev", "copy_occ", "total_kmers", "total_hits", "kernel_ms", "kernel_parts_ms", "algo_bytes", "free")}


def c_fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr, re.S).group(1), flags=re.S)
    return [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert set(re.findall(r"\b(kmx_kset_\w+)\s*\(", hdr)) == KSET
    assert set(re.findall(r"\b(kmx_match_\w+)\s*\(", hdr)) == MATCH
    from kmtricks_amd import lib
    assert set(lib.KSET_EXPORTS) == KSET and set(lib.MATCH_EXPORTS) == MATCH
    top = hdr[:hdr.index("#ifndef KMX_H")]
    assert "kmx_kset_dev / _host" in top and "kmx_match_dev / _host" in top
    assert "/* ------------------------------------------------------------------- kset */" in hdr
    assert "/* ------------------------------------------------------------------ match */" in hdr
    assert c_fields(hdr, "kmx_kset_task") == [f[0] for f in lib.KmxKsetTask._fields_]
    assert c_fields(hdr, "kmx_match_task") == [f[0] for f in lib.KmxMatchTask._fields_]
    assert c_fields(hdr, "kmx_match_rec") == list(lib.MATCH_REC.names)
    assert "16 to 32 bytes a key" in hdr and "#define KMX_MATCH_IDS 1u" in hdr and "#define KMX_MATCH_OCC 2u" in hdr


def test_library_and_binding_structures():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    for name in sorted(KSET | MATCH):
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxKsetTask) == 32 and lib.KmxKsetTask.kmer_size.offset == 16 and lib.KmxKsetTask.flags.offset == 24
    assert ctypes.sizeof(lib.KmxMatchTask) == 56 and lib.KmxMatchTask.n_seqs.offset == 24 and lib.KmxMatchTask.flags.offset == 32 and lib.KmxMatchTask.occ.offset == 40
    assert lib.MATCH_REC.itemsize == 24 and (lib.MATCH_IDS, lib.MATCH_OCC) == (1, 2)
    csrc = os.path.join(ROOT, "kmtricks_amd", "csrc")
    src = open(os.path.join(csrc, "match.hip")).read()
    for text in ("static_assert(sizeof(kmx_kset_task) == 32", "static_assert(sizeof(kmx_match_task) == 56", "static_assert(sizeof(kmx_match_rec) == 24",
                 'kmx_env_cus("KMX_MATCH_CUS", ctx)', 'kmx_env_grid("KMX_MATCH_GRID", planned)', 'kmx_env_int("KMX_MATCH_HASH_BITS")',
                 "q_tile_kmer_strand<KW>(", "q_tile_query(", "seq_n_bases(", "seq_args("):
        assert text in src, text
    assert "match.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "kmx_match.cpp" in open(os.path.join(ROOT, "kmtricks_amd", "host", "Makefile")).read()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def test_usage_is_pinned():
    r = kmx("match")
    assert r.returncode == 1 and r.stdout == "" and "usage: " + USAGE in r.stderr
    for word in ("Paired reads, approximate matching and per-read distinct counts are not done", "The set must fit one device"):
        assert word in r.stderr
    assert USAGE.replace("|", "\\|") in open(os.path.join(ROOT, "README.md")).read()      # (a table cell escapes the bar)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import random
    d = tmp_path_factory.mktemp("kmxmatch")
    rng = random.Random(2)
    seq = mr.rand_seq(rng, 120)
    (d / "reads.fa").write_text(f">r0 first\n{seq}\n>r1\n{mr.rand_seq(rng, 40)}\n")
    (d / "k.tsv").write_text("#c\nkmer\tp\n" + "".join(seq[i:i + 31] + "\t0.1\n" for i in range(0, 60, 7)))
    (d / "s.fa").write_text(f">0 LN:i:50\n{seq[:50]}\n")
    body = dr.make_body(0, 20, 3, 1, dr.MODE_COUNT)
    runs = {m: dr.write_run(d / m.replace(":", "_"), m, 31, ["A", "B", "C"], [body], window=16) for m in ("kmer:count:bin", "hash:count:bin", "hash:pa:bin")}
    return dict(dir=d, reads=d / "reads.fa", kmers=d / "k.tsv", seqs=d / "s.fa", runs=runs, body=body)


def refused(tmp_path, *args, text=None, outputs=True):
    outs = [tmp_path / "out.tsv", tmp_path / "ext.fa", tmp_path / "counts.tsv", tmp_path / "pos.tsv"]
    given = ["--output", outs[0], "--extract", outs[1], "--kmer-counts", outs[2], "--positions", outs[3]] if outputs else []
    r = kmx("match", *given, *args)
    assert r.returncode == 1 and r.stderr.startswith("[error] ") and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert text is None or r.stderr.startswith("[error] " + text), (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert not any(os.path.exists(p) for p in outs), "a refusal wrote a file"


def test_driver_refuses_bad_options(files, tmp_path):
    km, rd = ["--kmers", files["kmers"]], ["--reads", files["reads"]]
    refused(tmp_path, *rd, text="exactly one of --kmers, --seqs and --run is required\nusage: " + USAGE)
    refused(tmp_path, *km, *rd, "--seqs", files["seqs"], "--kmer-size", 31, text="exactly one of --kmers, --seqs and --run is required\n")
    refused(tmp_path, *km, *rd, "--run", files["runs"]["kmer:count:bin"], text="exactly one of --kmers, --seqs and --run is required\n")
    refused(tmp_path, *km, *rd, "--frobnicate", text="unknown option --frobnicate\nusage: " + USAGE)
    refused(tmp_path, *km, text="--reads is required\nusage: " + USAGE)
    refused(tmp_path, *km, *rd, text="one of --output, --extract, --kmer-counts and --positions is required\nusage: " + USAGE, outputs=False)
    refused(tmp_path, "--seqs", files["seqs"], *rd, text="--seqs needs --kmer-size\n")
    for k in (7, 128):
        refused(tmp_path, "--seqs", files["seqs"], "--kmer-size", k, *rd, text="--kmer-size must be in [8, 127]\n")
    refused(tmp_path, *km, "--kmer-size", 31, *rd, text="--kmer-size goes with --seqs")
    for opt in (["--min-hits", 2], ["--min-frac", 0.5], ["--min-cover", 0.5], ["--invert"]):
        refused(tmp_path, *km, *rd, "--output", tmp_path / "o.tsv", *opt, text="--min-hits, --min-frac, --min-cover and --invert need --extract\n", outputs=False)
    refused(tmp_path, *km, *rd, "--min-frac", 1.5, text="--min-frac must be inside [0, 1]\n")
    refused(tmp_path, *km, *rd, "--min-cover", "-0.1", text="--min-cover must be inside [0, 1]\n")
    refused(tmp_path, *km, *rd, "--min-frac", "half", text="bad number for --min-frac: half\n")
    refused(tmp_path, *km, *rd, "--min-hits", "-1", text="bad number for --min-hits: -1\n")
    refused(tmp_path, *km, *rd, "--min-hits", 2 ** 32, text="--min-hits does not fit 32 bits\n")
    for g in (0, 17):
        refused(tmp_path, *km, *rd, "--gpus", g, text="--gpus must be in [1, 16]\n")
    refused(tmp_path, *km, *rd, "--batch-mb", 4096, text="--batch-mb must be below 4096")
    refused(tmp_path, *km, "--reads", text="missing value for --reads\n")
    refused(tmp_path, *km, "--reads", tmp_path / "none.fa", text=f"Unable to read at {tmp_path / 'none.fa'}\n")
    refused(tmp_path, *km, *rd, "--reads", tmp_path / "none.fq", text=f"Unable to read at {tmp_path / 'none.fq'}\n")
    refused(tmp_path, "--kmers", tmp_path / "none.tsv", *rd, text=f"Unable to read at {tmp_path / 'none.tsv'}\n")
    refused(tmp_path, "--seqs", tmp_path / "none.fa", "--kmer-size", 31, *rd, text=f"Unable to read at {tmp_path / 'none.fa'}\n")
    refused(tmp_path, "--run", tmp_path / "nothing", *rd, text=f"{tmp_path / 'nothing'} is not a kmtricks runtime directory.\n")


def test_driver_refuses_runs_whose_keys_are_no_kmers(files, tmp_path):
    for mode in ("hash:count:bin", "hash:pa:bin"):
        refused(tmp_path, "--run", files["runs"][mode], "--reads", files["reads"],
                text="kmx match needs a run made with --mode kmer:count:bin or kmer:pa:bin (the keys of hash and Bloom filter runs are not k-mers)")
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text"):
        root = dr.write_run(files["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, ["A", "B", "C"], [files["body"]], options_mode=said)
        refused(tmp_path, "--run", root, "--reads", files["reads"], text="kmx match needs a run made with")


@pytest.mark.parametrize("text,word", [("ACGT\n", "line 1: a k-mer of 4 characters: k must be in [8, 127]"), ("A" * 128 + "\n", "line 1: a k-mer of 128 characters: k must be in [8, 127]"),
                                       ("#c\n" + "A" * 31 + "\n" + "A" * 32 + "\tx\n", "line 3: a k-mer of 32 characters, the first has 31"),
                                       ("A" * 30 + "N\t1\n", "line 1: malformed k-mer"), ("A" * 31 + "\n\n" + "A" * 15 + "-" + "C" * 15 + "\n", "line 3: malformed k-mer"),
                                       ("A" * 31 + " 3\n", "line 1: malformed k-mer"), ("# nothing\nkmer\tp\n", "names no k-mer")])
def test_driver_refuses_malformed_kmer_lists(files, tmp_path, text, word):
    with open(tmp_path / "k.tsv", "w") as f:
        f.write(text)
    refused(tmp_path, "--kmers", tmp_path / "k.tsv", "--reads", files["reads"], text=f"{tmp_path / 'k.tsv'} {word}")
    if word.startswith("line") and "[8, 127]" not in word:
        with pytest.raises(ValueError):
            mr.parse_kmers(text)


# ---- parsers and formats restated ------------------------------------------------------------------------------------------------------
def test_kmers_parser_restated():
    """the first tab-separated field, # lines, empty lines and the header line skipped, either strand and either case, CRLF, duplicates kept"""
    s = "ACGTTGCAAGGCTTAACCGGTTACGATCGAT"
    text = f"# kmx diff\nkmer\tpvalue\n{s}\n{mr.rc_str(s).lower()}\tcase\t0.1\r\n\n{'C' * 31}\tx\n{s}\n"
    k, got = mr.parse_kmers(text)
    c = mr.canon_of(s)
    assert k == 31 and got == [c, c, mr.canon_of("C" * 31), c]


def test_records_parser_restated():
    fa, fq = ">a one\nACGT\nacgt\n>b\n\n>c\r\nTT TT\r\n", "@q1 x y\nAC\nGT\n+\nII\nII\n@q2\nAAAA\n+q2\n@@@@\r\n"
    assert mr.parse_records(fa) == [(">a one", "ACGTacgt", None), (">b", "", None), (">c", "TTTT", None)]
    assert mr.parse_records(fq) == [("@q1 x y", "ACGT", "IIII"), ("@q2", "AAAA", "@@@@")]
    assert [mr.name_of(h) for h, _, _ in mr.parse_records(fa) + mr.parse_records(fq)] == ["a", "b", "c", "q1", "q2"]


def test_keep_rule_and_file_formats_restated():
    recs = [(10, 4, 3, 20, 2, 11), (10, 0, 0, 0, NONE, NONE), (0, 0, 0, 0, NONE, NONE), (4, 4, 0, 12, 0, 3)]
    reads, heads, quals = ["A" * 40, "C" * 40, "GG", "T" * 12], [">r0 x", ">r1", "@r2", "@r3 y z"], [None, None, "II", "J" * 12]
    assert [mr.kept(r, len(s)) for r, s in zip(recs, reads)] == [True, False, False, True]
    assert [mr.kept(r, len(s), invert=True) for r, s in zip(recs, reads)] == [False, True, True, False]
    assert [mr.kept(r, len(s), min_hits=0) for r, s in zip(recs, reads)] == [True, True, True, True]
    assert [mr.kept(r, len(s), min_hits=0, min_frac=0.0) for r, s in zip(recs, reads)] == [True, True, False, True]      # kmers > 0 when a fraction is given
    assert [mr.kept(r, len(s), min_frac=0.4) for r, s in zip(recs, reads)] == [True, False, False, True]
    assert [mr.kept(r, len(s), min_frac=0.41) for r, s in zip(recs, reads)] == [False, False, False, True]
    assert [mr.kept(r, len(s), min_cover=0.5) for r, s in zip(recs, reads)] == [True, False, False, True]
    assert [mr.kept(r, len(s), min_cover=0.51, invert=True) for r, s in zip(recs, reads)] == [True, True, True, False]
    assert mr.output_text(heads, reads, recs) == (mr.HEADER + "0\tr0\t40\t10\t4\t3\t20\t2\t11\n1\tr1\t40\t10\t0\t0\t0\t-\t-\n2\tr2\t2\t0\t0\t0\t0\t-\t-\n"
                                                  "3\tr3\t12\t4\t4\t0\t12\t0\t3\n")
    assert mr.HEADER == "read\tname\tlength\tkmers\thits\tfwd\tcovered\tfirst\tlast\n"
    assert mr.extract_text(heads, reads, quals, recs) == (f">r0 x KM:i:10 HT:i:4 FW:i:3 CV:i:20\n{'A' * 40}\n@r3 y z KM:i:4 HT:i:4 FW:i:0 CV:i:12\n{'T' * 12}\n+\n{'J' * 12}\n")
    e = mr.EXAMPLE
    r = mr.match_strings(list(e["keys"]), 5, list(e["reads"]))
    assert mr.kmer_counts_text(list(e["keys"]), 5, r.key_ids, r.occ) == "kmer\tcount\nTTGCA\t3\nATTGC\t2\nTGCAC\t2\n"
    assert mr.positions_text(5, list(e["reads"]), r.ids) == ("read\tpos\tkmer_index\tstrand\n0\t1\t1\t+\n0\t2\t0\t+\n0\t3\t3\t+\n1\t0\t0\t+\n1\t6\t0\t-\n1\t7\t1\t-\n4\t0\t3\t+\n")
