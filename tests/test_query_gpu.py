"""`kmx query` on the MI355X against tests/query_ref.py (the definition restated with Python integers and a dictionary per query):
the C ABI through kmtricks_amd.lib on synthetic indexes -- exact equality of n_kmers and hits --, and the driver on the golden
samples.  Run with -m gpu."""
import os, struct, subprocess
import numpy as np
import pytest

import orc
import query_ref as qr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def check(ctx, seqs, k, m, rep, W, N, mats, what="", bulk=False):
    en, eh = (qr.query_expected_bulk if bulk else qr.query_expected)(seqs, k, m, rep, W, N, mats)
    out = ctx.query(seqs, k, m, rep, W, N, mats)
    assert np.array_equal(out.n_kmers, en), f"{what}: n_kmers differ at queries {np.nonzero(out.n_kmers != en)[0][:8]}"
    bad = np.argwhere(out.hits != eh)
    assert not len(bad), f"{what}: hits differ in {len(bad)} cells, first (query, sample) {bad[:4].tolist()}: got {[int(out.hits[tuple(b)]) for b in bad[:4]]}, expected {[int(eh[tuple(b)]) for b in bad[:4]]}"
    return out


@pytest.fixture(scope="module")
def column_reads():
    return qr.random_reads(5, 300, 150)


@pytest.mark.parametrize("N", [1, 7, 8, 9, 63, 64, 65, 100, 513, 2500])
def test_columns(ctx, column_reads, N):
    """every width of a row around the byte, dword and 64-dword edges; every padding bit of every row is 1 in the input"""
    mats, rep = qr.synth_index(100 + N, N, 4099, 4, 31, 10, 0.3 if N <= 100 else 0.05, pad_ones=True)
    if N % 8:
        assert all((mt[:, -1] >> (N % 8)).min() == (0xFF >> (N % 8)) for mt in mats)
    check(ctx, column_reads, 31, 10, rep, 4099, N, mats, f"N={N}", bulk=N > 100)


@pytest.mark.parametrize("k", [12, 21, 31, 32, 33, 63, 64, 96, 127])
def test_kmer_sizes(ctx, k):
    """one to four key words, both sides of every word edge, the window of m-mers from 5 to 118"""
    m = 8 if k == 12 else 10
    mats, rep = qr.synth_index(k, 65, 10007, 8, k, m, 0.3)
    reads = qr.random_reads(k, 40, 150) + qr.random_reads(k + 1, 2, 700)
    check(ctx, reads, k, m, rep, 10007, 65, mats, f"k={k}")


def test_query_shapes(ctx):
    k, m, W, N, P = 31, 10, 4099, 65, 4
    mats, rep = qr.synth_index(9, N, W, P, k, m, 0.4)
    rnd = lambda seed, n: qr.random_reads(seed, 1, n)[0]
    unit = rnd(20, 30)
    seqs = ["", rnd(1, k - 1), rnd(2, k), rnd(3, k + 1),
            rnd(4, 63 + k - 1), rnd(5, 64 + k - 1), rnd(6, 65 + k - 1),               # 63, 64, 65 positions; 64 + k - 1 bases: the tile edge
            "N" + rnd(7, 99), rnd(8, 99) + "N", "N".join(rnd(30 + i, k - 1) for i in range(6)),      # an N at base 0, at the last base, at every k-th base
            rnd(9, 200).lower(), "A" * 120, (unit * 10)[:300], "", rnd(10, 5)]
    out = check(ctx, seqs, k, m, rep, W, N, mats, "shapes")
    assert out.n_kmers[0] == 0 and out.n_kmers[1] == 0 and out.n_kmers[2] == 1 and out.n_kmers[3] == 2
    assert list(out.n_kmers[4:7]) == [63, 64, 65] and out.n_kmers[9] == 0 and not out.hits[9].any()
    assert out.n_kmers[7] == 100 - k and out.n_kmers[8] == 100 - k and out.n_kmers[11] == 120 - k + 1


def test_counter_width(ctx):
    """one 70 000-base query, one partition of 257 rows: sums far past 65 535"""
    k, m, W, N = 31, 10, 257, 9
    seq = qr.random_reads(77, 1, 70000)
    rep = orc.repart_static(m, 1)
    ones, zeros, col8 = np.full((W, 2), 0xFF, np.uint8), np.zeros((W, 2), np.uint8), np.zeros((W, 2), np.uint8)
    col8[:, 1] = 1
    out = ctx.query(seq, k, m, rep, W, N, [ones])
    n = 70000 - k + 1
    assert out.n_kmers[0] == n > 65535 and (out.hits[0] == n).all()
    out = ctx.query(seq, k, m, rep, W, N, [zeros])
    assert out.n_kmers[0] == n and not out.hits.any()
    out = ctx.query(seq, k, m, rep, W, N, [col8])
    assert out.n_kmers[0] == n and out.hits[0, 8] == n and not out.hits[0, :8].any()
    # (and a matrix with something to get wrong, against the restatement)
    mats, _ = qr.synth_index(3, N, W, 1, k, m, 0.5, pad_ones=True)
    check(ctx, seq, k, m, rep, W, N, mats, "70 000 bases")


@pytest.fixture(scope="module")
def balance():
    k, m, W, N, P = 31, 10, 65521, 100, 32
    mats, rep = qr.synth_index(21, N, W, P, k, m, 0.2, pad_ones=True)
    seqs = qr.random_reads(22, 1, 2_000_000) + qr.random_reads(23, 5000, 100)
    en, eh = qr.query_expected_bulk(seqs, k, m, rep, W, N, mats)
    return dict(k=k, m=m, W=W, N=N, P=P, mats=mats, rep=rep, seqs=seqs, en=en, eh=eh)


def test_balance(ctx, balance):
    """one 2-Mbp query beside 5 000 reads of 100 bp, host and device-resident inputs"""
    import torch
    from kmtricks_amd import lib
    b = balance
    out = ctx.query(b["seqs"], b["k"], b["m"], b["rep"], b["W"], b["N"], b["mats"])
    assert np.array_equal(out.n_kmers, b["en"]) and np.array_equal(out.hits, b["eh"])
    assert out.algo_bytes == sum(len(s) for s in b["seqs"]) + int(b["en"].sum(dtype=np.uint64)) * 13 + 4 * len(b["seqs"]) * b["N"]
    blob, offs = lib.Context.pack_reads(b["seqs"])
    dev = torch.device("cuda:0")
    d_b = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_r = torch.from_numpy(b["rep"].view(np.int16)).to(dev)
    d_m = [torch.from_numpy(mt).to(dev) for mt in b["mats"]]
    torch.cuda.synchronize()
    out = ctx.query_dev(d_b.data_ptr(), d_o.data_ptr(), len(offs) - 1, b["k"], b["m"], d_r.data_ptr(), b["W"], b["N"], [t.data_ptr() for t in d_m])
    assert np.array_equal(out.n_kmers, b["en"]) and np.array_equal(out.hits, b["eh"])


def test_partition_groups(ctx, balance):
    """half the partitions, then the other half added into the same device table: the one-call table, n_kmers the same in all three"""
    b = balance
    even = [mt if p % 2 == 0 else None for p, mt in enumerate(b["mats"])]
    odd = [mt if p % 2 == 1 else None for p, mt in enumerate(b["mats"])]
    r1 = ctx.query(b["seqs"], b["k"], b["m"], b["rep"], b["W"], b["N"], even, keep=True)
    try:
        o1 = r1.output()
        assert np.array_equal(o1.n_kmers, b["en"]) and not np.array_equal(o1.hits, b["eh"])
        o2 = ctx.query(b["seqs"], b["k"], b["m"], b["rep"], b["W"], b["N"], odd, hits_dev=r1.hits_dev())
        assert np.array_equal(o2.n_kmers, b["en"]) and np.array_equal(o2.hits, b["eh"])
        assert np.array_equal(r1.output().hits, b["eh"])
    finally:
        r1.free()


@pytest.mark.parametrize("W,P", [(1, 1), (2, 1), (255, 256), (256, 1), (2 ** 20 + 7, 1), (2 ** 20 + 7, 256)])
def test_window_edges(ctx, W, P):
    k, m, N = 31, 10, 9
    big = W > 256
    mats, rep = qr.synth_index(W % 1000 + P, N, W, 1, k, m, 0.5, pad_ones=True)
    mats = mats * P if big else qr.synth_index(W + P, N, W, P, k, m, 0.5, pad_ones=True)[0]      # (256 windows of 2^20 rows share one body)
    rep = orc.repart_static(m, P)
    assert P == 1 or int(rep.max()) == P - 1
    check(ctx, qr.random_reads(W % 97 + P, 60, 120), k, m, rep, W, N, mats, f"W={W} P={P}")


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    rep = orc.repart_static(10, 1)
    for kw in (dict(k=7), dict(k=128), dict(m=3), dict(W=2 ** 32)):
        with pytest.raises(lib.KmxError):
            ctx.query(["ACGT" * 20], kw.get("k", 31), kw.get("m", 10), rep, kw.get("W", 64), 8, [None])


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    """`kmx pipeline --mode hash:bf:bin --hard-min 1` over the two golden samples, with the fixture's repartition table"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxquery")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    r = kmx(*base, "--run-dir", d / "bf", "--mode", "hash:bf:bin", "--bloom-size", 4000000)
    assert r.returncode == 0, r.stderr
    hi = open(d / "bf" / "hash.info", "rb").read()
    P, W = struct.unpack_from("<QQ", hi, 8)
    assert P == 4
    mats = []
    for p in range(P):
        raw = open(d / "bf" / "matrices" / f"matrix_{p}.cmbf", "rb").read()
        assert struct.unpack_from("<I", raw, 21)[0] == 2 and len(raw) == 49 + W
        mats.append(np.frombuffer(raw[49:], np.uint8).reshape(W, 1))
    return dict(dir=d, run=d / "bf", base=base, W=W, mats=mats, rep=t)


@pytest.fixture(scope="module")
def golden_expected(golden_run):
    out = {}
    for s in (1, 2):
        recs = qr.read_fasta_named(os.path.join(GD, f"{s}.fasta"))
        n, h = qr.query_expected([r[1] for r in recs], 31, 10, golden_run["rep"], golden_run["W"], 2, golden_run["mats"])
        out[s] = ([r[0] for r in recs], n, h)
    return out


@pytest.mark.parametrize("sample", [1, 2])
def test_driver_matches_the_restatement(golden_run, golden_expected, sample, tmp_path):
    names, n, h = golden_expected[sample]
    q = os.path.join(GD, f"{sample}.fasta")
    r = kmx("query", "--index", golden_run["run"], "--query", q)      # matrix is the default format, standard output the default place
    assert r.returncode == 0, r.stderr
    assert r.stdout == qr.format_matrix(names, ["D1", "D2"], n, h)
    # no false negatives: every k-mer of a sample's own reads is in the sample's column
    rows = [line.split("\t") for line in r.stdout.splitlines()[1:]]
    assert len(rows) == len(names) and sum(int(x[1]) for x in rows) > 0
    assert all(x[1] == x[1 + sample] for x in rows)
    for T in (None, 0.0, 1.0):
        r = kmx("query", "--index", golden_run["run"], "--query", q, "--format", "list", "--output", tmp_path / "l.txt", *(() if T is None else ("--threshold", T)))
        assert r.returncode == 0, r.stderr
        assert open(tmp_path / "l.txt").read() == qr.format_list(names, ["D1", "D2"], n, h, 0.7 if T is None else T)


def test_driver_groups_and_shards(golden_run, golden_expected, tmp_path):
    """several partition groups and query batches (--query-batch-mb), two shards on one device (--gpus 2): the same text"""
    names, n, h = golden_expected[1]
    want = qr.format_matrix(names, ["D1", "D2"], n, h)
    q = os.path.join(GD, "1.fasta")
    r = kmx("query", "--index", golden_run["run"], "--query", q, "--query-batch-mb", 1, "-v")
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    import re
    mt = re.search(r"(\d+) partition groups a shard", r.stderr)
    assert mt and int(mt.group(1)) >= 3, r.stderr
    r = kmx("query", "--index", golden_run["run"], "--query", q, "--gpus", 2, "--query-batch-mb", 1)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    r = kmx("query", "--index", golden_run["run"], "--query", q, "--gpus", 2)
    assert r.returncode == 0 and r.stdout == want, r.stderr


def test_driver_errors(golden_run, tmp_path):
    import shutil
    q = os.path.join(GD, "1.fasta")

    def refused(index, word):
        r = kmx("query", "--index", index, "--query", q)
        assert r.returncode == 1 and "[error]" in r.stderr and word in r.stderr, (r.returncode, r.stderr)
        assert r.stdout == ""

    r = kmx(*golden_run["base"], "--run-dir", tmp_path / "count", "--mode", "kmer:count:bin")
    assert r.returncode == 0, r.stderr
    refused(tmp_path / "count", "hash:bf:bin")
    shutil.copytree(golden_run["run"], tmp_path / "gone")
    os.remove(tmp_path / "gone" / "matrices" / "matrix_2.cmbf")
    refused(tmp_path / "gone", "matrix_2.cmbf")
    shutil.copytree(golden_run["run"], tmp_path / "bits")
    with open(tmp_path / "bits" / "matrices" / "matrix_1.cmbf", "r+b") as f:
        f.seek(21); f.write(struct.pack("<I", 3))
    refused(tmp_path / "bits", "matrix_1.cmbf")


def test_driver_bad_options(golden_run):
    q = os.path.join(GD, "1.fasta")
    for extra in (("--gpus", 0), ("--gpus", 17), ("--threshold", 1.5), ("--format", "table")):
        r = kmx("query", "--index", golden_run["run"], "--query", q, *extra)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (extra, r.stderr)
