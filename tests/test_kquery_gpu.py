"""`kmx query --kmer-index` on the MI355X against tests/kquery_ref.py (the definition restated with Python integers and a dictionary
per partition): the C ABI through kmtricks_amd.lib on synthetic indexes built from the reads' own k-mers and their near misses --
exact equality of n_kmers, hits and sums --, and the driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, shutil, struct, subprocess
import numpy as np
import pytest

import orc
import kquery_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = kr.MODE_COUNT, kr.MODE_PA


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, mode, what):
    en, eh, es = exp
    assert np.array_equal(out.n_kmers, en), f"{what}: n_kmers differ at queries {np.nonzero(out.n_kmers != en)[0][:8]}"
    bad = np.argwhere(out.hits != eh)
    assert not len(bad), f"{what}: hits differ in {len(bad)} cells, first (query, sample) {bad[:4].tolist()}: got {[int(out.hits[tuple(b)]) for b in bad[:4]]}, expected {[int(eh[tuple(b)]) for b in bad[:4]]}"
    if mode == COUNT:
        bad = np.argwhere(out.sums != es)
        assert not len(bad), f"{what}: sums differ in {len(bad)} cells, first (query, sample) {bad[:4].tolist()}: got {[int(out.sums[tuple(b)]) for b in bad[:4]]}, expected {[int(es[tuple(b)]) for b in bad[:4]]}"


def check(ctx, seqs, k, m, rep, N, mode, mats, what="", bulk=False, at=None):
    exp = kr.kquery_expected_bulk(seqs, k, m, rep, N, mode, mats) if bulk else kr.kquery_expected(seqs, k, m, rep, N, mode, mats, at=at)
    out = ctx.kquery(seqs, k, m, rep, N, orc.kw_of_k(k), mode, mats, sums=mode == COUNT)
    same(out, exp, mode, what)
    return out, exp


@pytest.fixture(scope="module")
def col():
    """300 reads of 150 bases, k 31, four partitions: their k-mers per partition and every position's place, worked out once"""
    k, m, P = 31, 10, 4
    reads = kr.random_reads(5, 300, 150)
    rep = orc.repart_static(m, P)
    return dict(k=k, m=m, P=P, reads=reads, rep=rep, keys=kr.read_keys(reads, k, m, rep, P), at=kr.places(reads, k, m, rep))


@pytest.mark.parametrize("N", [1, 7, 8, 9, 63, 64, 65, 100, 513, 2500])
def test_columns_pa(ctx, col, N):
    """every width of a row around the byte, dword and 64-dword edges -- rows of 8 + ceil(N / 8) bytes start at every alignment --; every
    padding bit of every row is 1 in the input"""
    mats, rep = kr.synth_kindex(100 + N, N, col["P"], col["k"], col["m"], PA, col["reads"], 0.7, pad_ones=True, fill=0.3 if N <= 100 else 0.05, keys=col["keys"])
    if N % 8:
        assert all((kr.split_matrix(mt, col["k"], N, PA)[1][:, -1] >> (N % 8)).min() == (0xFF >> (N % 8)) for mt in mats)
    out, exp = check(ctx, col["reads"], col["k"], col["m"], rep, N, PA, mats, f"PA N={N}", bulk=N > 100, at=col["at"])
    assert exp[1].any()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 2500])
def test_columns_count(ctx, col, N):
    """one lane group, both sides of 64 lanes, more than one pass of 4 x 64 columns; zero counts inside kept rows, counts of 0xFFFFFFFF"""
    mats, rep = kr.synth_kindex(200 + N, N, col["P"], col["k"], col["m"], COUNT, col["reads"], 0.7, zeros=0.2, maxed=0.02, keys=col["keys"])
    out, exp = check(ctx, col["reads"], col["k"], col["m"], rep, N, COUNT, mats, f"COUNT N={N}", bulk=N > 100, at=col["at"])
    assert exp[1].any() and int(exp[2].max()) >= 0xFFFFFFFF


@pytest.mark.parametrize("mode", [COUNT, PA])
@pytest.mark.parametrize("k", [12, 31, 32, 33, 63, 64, 96, 127])
def test_kmer_sizes(ctx, k, mode):
    """one to four key words, both sides of every word edge; the reads share their first 40 bases, so many keys share their upper words,
    and three rows in ten are near misses (key - 1, key + 1) of a k-mer of the reads"""
    m, N, P = (8 if k == 12 else 10), (5 if mode == COUNT else 65), 8
    reads = ["A" * 40 + r for r in kr.random_reads(k, 40, 110)] + ["A" * 40 + r for r in kr.random_reads(k + 1, 2, 660)]
    mats, rep = kr.synth_kindex(k, N, P, k, m, mode, reads, 0.8, near=0.3, pad_ones=True, zeros=0.1)
    out, exp = check(ctx, reads, k, m, rep, N, mode, mats, f"k={k} mode={mode}")
    assert exp[1].any()


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_search_edges(ctx, col, mode):
    """a partition of no rows, one of one row, one without its first and last key (the queries hold a k-mer below the first row, one above
    the last, and the first and last rows' own), a partition that is not part of the call; an index of none and of all of the k-mers"""
    k, m, P, N, keys = col["k"], col["m"], col["P"], 9, col["keys"]
    rng = np.random.default_rng(7)
    pay = lambda n: (rng.integers(1, 50, (n, N)).astype(np.uint32).view(np.uint8).reshape(n, 4 * N) if mode == COUNT
                     else np.packbits(np.concatenate([rng.random((n, N)) < 0.5, np.ones((n, 7), bool)], axis=1), axis=1, bitorder="little"))
    assert all(len(x) > 10 for x in keys)
    mats = [kr.make_body([], pay(0), k), kr.make_body(keys[1][len(keys[1]) // 2:][:1], pay(1), k), kr.make_body(keys[2][1:-1], pay(len(keys[2]) - 2), k), None]
    out, exp = check(ctx, col["reads"], k, m, col["rep"], N, mode, mats, "edges", at=col["at"])
    assert exp[1].any()
    two = [None, None, kr.make_body([keys[2][0], keys[2][-1]], pay(2), k), None]      # a matrix of the least and the greatest k-mer alone
    out, exp = check(ctx, col["reads"], k, m, col["rep"], N, mode, two, "first and last", at=col["at"])
    assert exp[1].any()
    for frac in (0.0, 1.0):
        mats, rep = kr.synth_kindex(3, N, P, k, m, mode, col["reads"], frac, near=0.0, keys=keys)
        out, exp = check(ctx, col["reads"], k, m, rep, N, mode, mats, f"frac={frac}", at=col["at"])
        if frac == 0.0:
            assert all(len(mt) == 0 for mt in mats) and not out.hits.any()
        elif mode == COUNT:
            assert (out.hits == out.n_kmers[:, None]).all()      # every k-mer is a row, no count is zero


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_query_shapes(ctx, mode):
    k, m, N, P = 31, 10, 65, 4
    rnd = lambda seed, n: kr.random_reads(seed, 1, n)[0]
    unit = rnd(20, 30)
    seqs = ["", rnd(1, k - 1), rnd(2, k), rnd(3, k + 1),
            rnd(4, 63 + k - 1), rnd(5, 64 + k - 1), rnd(6, 65 + k - 1),               # 63, 64, 65 positions; 64 + k - 1 bases: the tile edge
            "N" + rnd(7, 99), rnd(8, 99) + "N", "N".join(rnd(30 + i, k - 1) for i in range(6)),      # an N at base 0, at the last base, at every k-th base
            rnd(9, 200).lower(), "A" * 120, (unit * 10)[:300], "", rnd(10, 5)]
    mats, rep = kr.synth_kindex(9, N, P, k, m, mode, seqs, 0.8, near=0.1, pad_ones=True)
    out, exp = check(ctx, seqs, k, m, rep, N, mode, mats, "shapes")
    assert out.n_kmers[0] == 0 and out.n_kmers[1] == 0 and out.n_kmers[2] == 1 and out.n_kmers[3] == 2
    assert list(out.n_kmers[4:7]) == [63, 64, 65] and out.n_kmers[9] == 0 and not out.hits[9].any()
    assert out.n_kmers[7] == 100 - k and out.n_kmers[8] == 100 - k and out.n_kmers[11] == 120 - k + 1
    assert out.hits[10].any()      # lower case


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_counter_width(ctx, mode):
    """one k-mer 69 970 times: a hit sum past 65 535, a count sum past 2^32, a zero count in a found row"""
    k, m, N = 31, 10, 3
    seq = ["A" * 70000]
    n = 70000 - k + 1
    rep = orc.repart_static(m, 1)
    at = kr.places(seq, k, m, rep)
    assert len(at[0]) == n and len(set(at[0])) == 1 and at[0][0][1] == 0      # poly-A: the canonical k-mer is key 0
    if mode == COUNT:
        body = kr.make_body([0, 5], np.array([[0xFFFFFFFF, 0, 5], [1, 1, 1]], np.uint32).view(np.uint8).reshape(2, 12), k)
        out, exp = check(ctx, seq, k, m, rep, N, COUNT, [body], "poly-A", at=at)
        assert out.n_kmers[0] == n > 65535 and list(out.hits[0]) == [n, 0, n]
        assert list(out.sums[0]) == [n * 0xFFFFFFFF, 0, 5 * n] and int(out.sums[0, 0]) > 2 ** 32
    else:
        body = kr.make_body([0, 5], np.array([[0xFD], [0xFF]], np.uint8), k)      # bits 0 and 2, every padding bit
        out, exp = check(ctx, seq, k, m, rep, N, PA, [body], "poly-A", at=at)
        assert out.n_kmers[0] == n and list(out.hits[0]) == [n, 0, n]


@pytest.fixture(scope="module")
def balance():
    """one 2-Mbp query beside 5 000 reads of 100 bases: query changes fall inside the gather's runs; a fifth of their k-mers indexed"""
    k, m, N, P = 31, 10, 70, 8
    seqs = kr.random_reads(22, 1, 2_000_000) + kr.random_reads(23, 5000, 100)
    mats, rep = kr.synth_kindex(21, N, P, k, m, COUNT, seqs, 0.2, near=0.1, zeros=0.1)
    exp = kr.kquery_expected_bulk(seqs, k, m, rep, N, COUNT, mats)
    return dict(k=k, m=m, N=N, P=P, mats=mats, rep=rep, seqs=seqs, exp=exp)


def test_balance(ctx, balance):
    """host and device-resident inputs"""
    import torch
    from kmtricks_amd import lib
    b = balance
    out = ctx.kquery(b["seqs"], b["k"], b["m"], b["rep"], b["N"], 1, COUNT, b["mats"], sums=True)
    same(out, b["exp"], COUNT, "balance")
    stride = kr.stride_of(b["k"], b["N"], COUNT)
    found = out.algo_bytes - (sum(len(s) for s in b["seqs"]) + int(b["exp"][0].sum(dtype=np.uint64)) * 8 + 12 * len(b["seqs"]) * b["N"])
    assert found > 0 and found % stride == 0 and found // stride <= int(b["exp"][0].sum(dtype=np.uint64))
    blob, offs = lib.Context.pack_reads(b["seqs"])
    dev = torch.device("cuda:0")
    d_b = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_r = torch.from_numpy(b["rep"].view(np.int16)).to(dev)
    d_m = [torch.from_numpy(mt).to(dev) for mt in b["mats"]]
    torch.cuda.synchronize()
    out = ctx.kquery_dev(d_b.data_ptr(), d_o.data_ptr(), len(offs) - 1, b["k"], b["m"], d_r.data_ptr(), b["N"], 1, COUNT,
                         [t.data_ptr() for t in d_m], [len(mt) // stride for mt in b["mats"]], sums=True)
    same(out, b["exp"], COUNT, "balance, device-resident")


def test_partition_groups_count(ctx, balance):
    """half the partitions, then the other half added into the same device tables: the one-call tables, n_kmers the same in all three"""
    b = balance
    even = [mt if p % 2 == 0 else None for p, mt in enumerate(b["mats"])]
    odd = [mt if p % 2 == 1 else None for p, mt in enumerate(b["mats"])]
    r1 = ctx.kquery(b["seqs"], b["k"], b["m"], b["rep"], b["N"], 1, COUNT, even, sums=True, keep=True)
    try:
        o1 = r1.output()
        assert np.array_equal(o1.n_kmers, b["exp"][0]) and not np.array_equal(o1.hits, b["exp"][1])
        o2 = ctx.kquery(b["seqs"], b["k"], b["m"], b["rep"], b["N"], 1, COUNT, odd, hits_dev=r1.hits_dev(), sums=r1.sums_dev())
        same(o2, b["exp"], COUNT, "groups")
        same(r1.output(), b["exp"], COUNT, "groups, the first result")
    finally:
        r1.free()


def test_partition_groups_pa(ctx, col):
    mats, rep = kr.synth_kindex(31, 100, col["P"], col["k"], col["m"], PA, col["reads"], 0.7, pad_ones=True, keys=col["keys"])
    exp = kr.kquery_expected(col["reads"], col["k"], col["m"], rep, 100, PA, mats, at=col["at"])
    r1 = ctx.kquery(col["reads"], col["k"], col["m"], rep, 100, 1, PA, [mats[0], None, mats[2], None], keep=True)
    try:
        assert not np.array_equal(r1.output().hits, exp[1]) and r1.sums_dev() is None
        o2 = ctx.kquery(col["reads"], col["k"], col["m"], rep, 100, 1, PA, [None, mats[1], None, mats[3]], hits_dev=r1.hits_dev())
        same(o2, exp, PA, "PA groups")
    finally:
        r1.free()


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_many_partitions(ctx, col, mode):
    P, N = 256, 9
    mats, rep = kr.synth_kindex(4, N, P, col["k"], col["m"], mode, col["reads"], 0.7, pad_ones=True)
    assert int(rep.max()) == P - 1
    check(ctx, col["reads"], col["k"], col["m"], rep, N, mode, mats, f"P={P}")


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    INVAL, UNSUP = r"\(-2\)", r"\(-5\)"
    rep = orc.repart_static(10, 1)
    body = kr.make_body([1], np.ones((1, 4), np.uint8), 31)      # one COUNT row of one column

    def call(code, k=31, m=10, N=1, kw=1, mode=COUNT, mats=(body,), n_rows=(1,), sums=False):
        with pytest.raises(lib.KmxError, match=code):
            ctx.kquery(["ACGT" * 20], k, m, rep, N, kw, mode, list(mats), n_rows=n_rows, sums=sums)

    call(INVAL, k=7, kw=1); call(INVAL, k=128, kw=4)
    call(INVAL, m=3); call(INVAL, m=16); call(INVAL, k=12, m=12)
    call(INVAL, kw=2); call(INVAL, k=33, kw=1)                          # key_words == ceil(k / 32)
    call(INVAL, mats=[None] * 65536)
    call(INVAL, N=0)
    call(INVAL, mode=PA, sums=True, mats=(kr.make_body([1], np.ones((1, 1), np.uint8), 31),))
    call(INVAL, mode=7)
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode)
    call(UNSUP, n_rows=[2 ** 32 - 255])
    call(UNSUP, N=2 ** 30)                                   # a row of 8 + 2^32 bytes
    # 2^31 queries, 2^32 bases: refused from the numbers alone
    offs = np.array([0, 2 ** 32], np.uint64)
    rows, nr = (C.c_void_p * 1)(body.ctypes.data), (C.c_uint64 * 1)(1)
    for n_seqs, o in ((2 ** 31, offs), (1, offs)):
        t = lib.KmxKqueryTask(body.ctypes.data, o.ctypes.data, n_seqs, 31, 10, rep.ctypes.data, 1, 1, 1, COUNT, nr, rows, None, None, 0)
        res = C.c_void_p()
        assert lib._lib.kmx_kquery_host(ctx._h, C.byref(t), C.byref(res)) == -5 and not res.value
    # and the call that is inside every limit runs
    out = ctx.kquery(["ACGT" * 20], 31, 10, rep, 1, 1, COUNT, [body], sums=True)
    assert out.n_kmers[0] == 50 and not out.hits.any()


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples in kmer:count:bin and kmer:pa:bin, with the fixture's repartition table;
    the matrices as tests/kquery_ref.py reads them from the files"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxkquery")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    runs = {}
    for mode, name, ext in ((COUNT, "count", "count"), (PA, "pa", "pa")):
        r = kmx(*base, "--run-dir", d / name, "--mode", f"kmer:{name}:bin")
        assert r.returncode == 0, r.stderr
        files = [kr.read_matrix_file(d / name / "matrices" / f"matrix_{p}.{ext}") for p in range(4)]
        assert all(f["k"] == 31 and f["n_cols"] == 2 and f["mode"] == mode for f in files)
        runs[mode] = dict(run=d / name, mats=[f["body"] for f in files])
    return dict(dir=d, base=base, rep=t, runs=runs)


@pytest.fixture(scope="module")
def golden_expected(golden_runs):
    out = {}
    for s in (1, 2):
        recs = kr.read_fasta_named(os.path.join(GD, f"{s}.fasta"))
        seqs = [r[1] for r in recs]
        at = kr.places(seqs, 31, 10, golden_runs["rep"])
        for mode in (COUNT, PA):
            out[s, mode] = ([r[0] for r in recs], seqs) + kr.kquery_expected(seqs, 31, 10, golden_runs["rep"], 2, mode, golden_runs["runs"][mode]["mats"], at=at)
    return out


@pytest.mark.parametrize("mode", [COUNT, PA])
@pytest.mark.parametrize("sample", [1, 2])
def test_driver_matches_the_restatement(golden_runs, golden_expected, sample, mode, tmp_path):
    names, seqs, n, h, s = golden_expected[sample, mode]
    run = golden_runs["runs"][mode]["run"]
    q = os.path.join(GD, f"{sample}.fasta")
    r = kmx("query", "--kmer-index", run, "--query", q)      # matrix is the default format, standard output the default place
    assert r.returncode == 0, r.stderr
    assert r.stdout == kr.format_matrix(names, ["D1", "D2"], n, h)
    # without the restatement: the runs keep every k-mer (--hard-min 1), so every k-mer of a sample's own reads is in its column
    rows = [line.split("\t") for line in r.stdout.splitlines()[1:]]
    assert len(rows) == len(names) and sum(int(x[1]) for x in rows) > 0
    assert all(x[1] == x[1 + sample] for x in rows)
    for T in (None, 0.0, 1.0):
        r = kmx("query", "--kmer-index", run, "--query", q, "--format", "list", "--output", tmp_path / "l.txt", *(() if T is None else ("--threshold", T)))
        assert r.returncode == 0, r.stderr
        assert open(tmp_path / "l.txt").read() == kr.format_list(names, ["D1", "D2"], n, h, 0.7 if T is None else T)
    if mode == COUNT:
        r = kmx("query", "--kmer-index", run, "--query", q, "--format", "sums")
        assert r.returncode == 0, r.stderr
        assert r.stdout == kr.format_sums(names, ["D1", "D2"], n, s)


def test_driver_single_kmer_is_its_row(golden_runs, tmp_path):
    """a query of one k-mer: its sums are its matrix row"""
    k, mats = 31, golden_runs["runs"][COUNT]["mats"]
    picked = []
    for p in (0, 3):
        keys, pay = kr.split_matrix(mats[p], k, 2, COUNT)
        for r in (0, len(keys) // 2, len(keys) - 1):
            picked.append((orc.kmer_to_string(keys[r], k), [int(x) for x in np.ascontiguousarray(pay[r]).view(np.uint32)]))
    with open(tmp_path / "one.fa", "w") as f:
        for i, (kmer, _) in enumerate(picked):
            f.write(f">k{i}\n{kmer}\n")
    r = kmx("query", "--kmer-index", golden_runs["runs"][COUNT]["run"], "--query", tmp_path / "one.fa", "--format", "sums")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "query\tn_kmers\tD1\tD2\n" + "".join(f"k{i}\t1\t{row[0]}\t{row[1]}\n" for i, (_, row) in enumerate(picked))


@pytest.fixture(scope="module")
def big_run(golden_runs):
    """a count run whose matrices are larger than a partition group of --query-batch-mb 1: 4 000 random reads as one sample, golden
    sample 1 as the other, split with the static repartition table (the goldens' table sends nearly every k-mer of random reads to one
    partition); 300 of the reads, the golden reads and a stranger as queries, judged from the matrix files"""
    d = golden_runs["dir"]
    rep = orc.repart_static(10, 4)
    with open(d / "static.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(rep), 1)); f.write(rep.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    reads = kr.random_reads(41, 4000, 150)
    with open(d / "big.fasta", "w") as f:
        f.write("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    with open(d / "big.fof", "w") as f:
        f.write(f"S1 : {d}/big.fasta\nS2 : {GD}/1.fasta\n")
    base = [{"in.fof": d / "big.fof", "fixture.minimRepart": d / "static.minimRepart"}.get(os.path.basename(str(a)), a) for a in golden_runs["base"]]
    r = kmx(*base, "--run-dir", d / "big", "--mode", "kmer:count:bin")
    assert r.returncode == 0, r.stderr
    mats = [kr.read_matrix_file(d / "big" / "matrices" / f"matrix_{p}.count")["body"] for p in range(4)]
    assert min(len(mt) for mt in mats) > (1 << 19)      # every matrix is a group of its own at 1 MB
    gold = kr.read_fasta_named(os.path.join(GD, "1.fasta"))
    queries = [(f"r{i}", reads[i]) for i in range(0, 3000, 10)] + gold + [("stranger", kr.random_reads(42, 1, 500)[0])]
    with open(d / "big_q.fasta", "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in queries))
    n, h, s = kr.kquery_expected_bulk([q[1] for q in queries], 31, 10, rep, 2, COUNT, mats)
    assert (h[:300, 0] == n[:300]).all() and not h[-1].any()
    return dict(run=d / "big", query=d / "big_q.fasta", names=[q[0] for q in queries], n=n, h=h, s=s)


def test_driver_groups_and_shards(big_run):
    """several partition groups and query batches (--query-batch-mb), two shards on one device (--gpus 2): the same text"""
    import re
    b = big_run
    for fmt, want in (("matrix", kr.format_matrix(b["names"], ["S1", "S2"], b["n"], b["h"])), ("sums", kr.format_sums(b["names"], ["S1", "S2"], b["n"], b["s"]))):
        r = kmx("query", "--kmer-index", b["run"], "--query", b["query"], "--format", fmt)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        r = kmx("query", "--kmer-index", b["run"], "--query", b["query"], "--format", fmt, "--query-batch-mb", 1, "-v")
        assert r.returncode == 0, r.stderr
        assert r.stdout == want
        mt = re.search(r"(\d+) query batches, (\d+) partition groups a shard", r.stderr)
        assert mt and int(mt.group(1)) >= 2 and int(mt.group(2)) >= 3, r.stderr
        r = kmx("query", "--kmer-index", b["run"], "--query", b["query"], "--format", fmt, "--gpus", 2, "--query-batch-mb", 1)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        r = kmx("query", "--kmer-index", b["run"], "--query", b["query"], "--format", fmt, "--gpus", 2)
        assert r.returncode == 0 and r.stdout == want, r.stderr


def test_driver_lz4(golden_runs, golden_expected, tmp_path):
    """a run written with --cpr gives the same text"""
    q = os.path.join(GD, "1.fasta")
    for mode, name in ((COUNT, "count"), (PA, "pa")):
        r = kmx(*golden_runs["base"], "--run-dir", tmp_path / f"lz_{name}", "--mode", f"kmer:{name}:bin", "--cpr")
        assert r.returncode == 0, r.stderr
        assert os.path.exists(tmp_path / f"lz_{name}" / "matrices" / f"matrix_0.{name}.lz4")
        names, seqs, n, h, s = golden_expected[1, mode]
        r = kmx("query", "--kmer-index", tmp_path / f"lz_{name}", "--query", q)
        assert r.returncode == 0 and r.stdout == kr.format_matrix(names, ["D1", "D2"], n, h), r.stderr


def test_driver_refusals(golden_runs, tmp_path):
    q = os.path.join(GD, "1.fasta")
    count, pa = golden_runs["runs"][COUNT]["run"], golden_runs["runs"][PA]["run"]

    def refused(*args, word=None):
        r = kmx("query", *args, "--query", q)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
        assert word is None or word in r.stderr, (args, r.stderr)

    r = kmx(*golden_runs["base"], "--run-dir", tmp_path / "bf", "--mode", "hash:bf:bin", "--bloom-size", 4000000)
    assert r.returncode == 0, r.stderr
    refused("--kmer-index", tmp_path / "bf", word="kmer:count:bin")
    shutil.copytree(count, tmp_path / "cut")
    with open(tmp_path / "cut" / "matrices" / "matrix_2.count", "r+b") as f:
        f.truncate(os.path.getsize(tmp_path / "cut" / "matrices" / "matrix_2.count") - 3)
    refused("--kmer-index", tmp_path / "cut", word="matrix_2.count")
    shutil.copytree(pa, tmp_path / "gone")
    os.remove(tmp_path / "gone" / "matrices" / "matrix_1.pa")
    refused("--kmer-index", tmp_path / "gone", word="matrix_1.pa")
    shutil.copytree(count, tmp_path / "cols")
    with open(tmp_path / "cols" / "matrices" / "matrix_0.count", "r+b") as f:
        f.seek(33); f.write(struct.pack("<I", 3))
    refused("--kmer-index", tmp_path / "cols", word="matrix_0.count")
    refused("--kmer-index", count, "--index", count)
    refused()
    refused("--kmer-index", pa, "--format", "sums", word="sums")
    refused("--index", count, word="hash:bf:bin")      # as before: a k-mer run is not a Bloom index
