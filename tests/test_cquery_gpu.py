"""`kmx query` over a counting Bloom index on the MI355X against tests/cquery_ref.py: the C ABI through kmtricks_amd.lib on synthetic
indexes -- exact equality of n_kmers, hits and sums --, and the driver on the golden samples, cross-checked against a hash:count:bin
run of the same samples.  Run with -m gpu."""
import ctypes as C
import os, re, shutil, struct, subprocess
import numpy as np
import pytest

import orc
import query_ref as qr
import cquery_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
K, M, P, W = 31, 10, 4, 4099


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, what):
    en, eh, es = exp
    assert np.array_equal(out.n_kmers, en), f"{what}: n_kmers differ at queries {np.nonzero(out.n_kmers != en)[0][:8]}"
    for name, got, want in (("hits", out.hits, eh), ("sums", out.sums, es)):
        bad = np.argwhere(got != want)
        assert not len(bad), f"{what}: {name} differ in {len(bad)} cells, first (query, sample) {bad[:4].tolist()}: got {[int(got[tuple(b)]) for b in bad[:4]]}, expected {[int(want[tuple(b)]) for b in bad[:4]]}"


@pytest.fixture(scope="module")
def col():
    """120 reads of 150 bases, k 31, four partitions of 4099 rows: every position's address, worked out once"""
    reads = qr.random_reads(5, 120, 150)
    rep = orc.repart_static(M, P)
    return dict(reads=reads, rep=rep, at=cr.np_addresses(reads, K, M, rep, W, P))


WS = (1, 2, 3, 4, 5, 7, 8)
NS = (1, 7, 8, 9, 63, 64, 65, 100, 513, 2500)      # 513: more than 64 blocks of 8 columns, a second pass
SHAPES = sorted({(N, WS[(i + j) % 7]) for i, N in enumerate(NS) for j in (0, 3)} | {(513, 3), (513, 8), (2500, 5), (65, 8), (9, 3)})


@pytest.mark.parametrize("N,w", SHAPES)
def test_columns(ctx, col, N, w):
    """every width of a row around the block, the 64-block and the byte edges, uniform classes; every padding bit of every row is 1"""
    mats, rep = cr.synth_index_bfc(100 * N + w, N, W, P, K, M, w, pad_ones=True)
    if (N * w) % 8:
        assert all((mt[:, -1] & (0xFF >> ((N * w) % 8))).min() == (0xFF >> ((N * w) % 8)) for mt in mats)
    n = 30 if N > 100 else len(col["reads"])      # (the wide rows: fewer reads, the same edges)
    for mc in sorted({1, min(2, (1 << w) - 1)}):
        exp = cr.np_expected_at(col["at"][:n], W, N, mats, w, mc)
        same(ctx.cquery(col["reads"][:n], K, M, rep, W, N, mats, w, min_class=mc), exp, f"N={N} w={w} min_class={mc}")
        assert exp[1].any() and exp[2].any()


@pytest.mark.parametrize("w", WS)
def test_bodies(ctx, col, w):
    """an all-zero body; a body of every bit set (the top class: 255 at w = 8, clamped); a body of classes that are all 1 asked for the
    top class: sums and no hit"""
    N, top, reads, rep = 13, (1 << w) - 1, col["reads"], col["rep"]
    n = np.full(len(reads), 150 - K + 1, np.uint32)
    mats, _ = cr.synth_index_bfc(1, N, W, P, K, M, w, dist="zero")
    out = ctx.cquery(reads, K, M, rep, W, N, mats, w)
    assert np.array_equal(out.n_kmers, n) and not out.hits.any() and not out.sums.any()
    mats, _ = cr.synth_index_bfc(1, N, W, P, K, M, w, dist="ones")
    for mc in (1, top):
        out = ctx.cquery(reads, K, M, rep, W, N, mats, w, min_class=mc)
        same(out, cr.np_expected_at(col["at"], W, N, mats, w, mc), f"ones w={w} min_class={mc}")
        assert (out.hits == n[:, None]).all() and (out.sums == n[:, None].astype(np.uint64) * cr.floor_of(top)).all()
    if w == 8:
        assert cr.floor_of(top) == 2 ** 31
    mats, _ = cr.synth_index_bfc(1, N, W, P, K, M, w, pad_ones=True, dist=1)
    if w > 1:
        out = ctx.cquery(reads, K, M, rep, W, N, mats, w, min_class=top)
        same(out, cr.np_expected_at(col["at"], W, N, mats, w, top), f"class 1 w={w}")
        assert not out.hits.any() and (out.sums == n[:, None]).all()


def test_flush_boundaries(ctx):
    """one query of 700 positions in a single partition (runs longer than the register window); many reads of k ... k + 2 bases (the
    query changes inside a run); empty reads and reads without a valid k-mer between them"""
    N, w = 21, 3
    rnd = lambda seed, n: qr.random_reads(seed, 1, n)[0]
    mats, rep = cr.synth_index_bfc(8, N, W, 1, K, M, w, pad_ones=True)
    seqs = [rnd(1, 700 + K - 1)]
    same(ctx.cquery(seqs, K, M, rep, W, N, mats, w), cr.cquery_expected_np(seqs, K, M, rep, W, N, mats, w), "one long query, one partition")
    mats, rep = cr.synth_index_bfc(9, N, W, P, K, M, w, pad_ones=True)
    seqs = []
    for i in range(400):
        seqs.append(rnd(100 + i, K + i % 3))
        if i % 7 == 0:
            seqs += ["", rnd(900 + i, K - 1), "ACGT" * 7 + "N" + "ACGT" * 7]
    exp = cr.cquery_expected(seqs, K, M, rep, W, N, mats, w)
    assert exp[0][0] == 1 and exp[0][1] == 0 and exp[0][2] == 0 and exp[0][3] == 0 and exp[0][4] == 2
    same(ctx.cquery(seqs, K, M, rep, W, N, mats, w), exp, "short reads")
    same(ctx.cquery(seqs, K, M, rep, W, N, mats, w, min_class=5), cr.cquery_expected_np(seqs, K, M, rep, W, N, mats, w, 5), "short reads, min_class 5")


def test_sums_past_32_bits(ctx):
    """w = 6, a body of class 32, a read of 200 valid positions: every sum is 200 * 2^31"""
    N, w = 9, 6
    mats, rep = cr.synth_index_bfc(2, N, W, P, K, M, w, pad_ones=True, dist=32)
    seqs = qr.random_reads(3, 1, 200 + K - 1)
    exp = cr.cquery_expected_np(seqs, K, M, rep, W, N, mats, w, 32)
    assert exp[0][0] == 200 and int(exp[2].min()) == 200 * 2 ** 31 >= 2 ** 32
    out = ctx.cquery(seqs, K, M, rep, W, N, mats, w, min_class=32)
    same(out, exp, "class 32")
    assert (out.hits == 200).all()


@pytest.mark.parametrize("k", [12, 31, 33, 64, 96, 127])
def test_kmer_sizes(ctx, k):
    m, N, w, Pk, Wk = (8 if k == 12 else 10), 65, 5, 8, 10007
    mats, rep = cr.synth_index_bfc(k, N, Wk, Pk, k, m, w, pad_ones=True)
    reads = qr.random_reads(k, 30, 150) + qr.random_reads(k + 1, 1, 700) + ["N" + qr.random_reads(k + 2, 1, 160)[0].lower(), "", "ACG"]
    same(ctx.cquery(reads, k, m, rep, Wk, N, mats, w, min_class=3), cr.cquery_expected_np(reads, k, m, rep, Wk, N, mats, w, 3), f"k={k}")


@pytest.fixture(scope="module")
def groups(col):
    N, w, mc = 100, 4, 2
    mats, rep = cr.synth_index_bfc(21, N, W, P, K, M, w, pad_ones=True)
    return dict(N=N, w=w, mc=mc, mats=mats, rep=rep, exp=cr.np_expected_at(col["at"], W, N, mats, w, mc))


def test_partition_groups(ctx, col, groups):
    """partitions that are not part of the call; half the partitions, then the other half added into the same two device tables: the
    one-call tables, n_kmers the same in all three"""
    g, reads = groups, col["reads"]
    even = [mt if p % 2 == 0 else None for p, mt in enumerate(g["mats"])]
    odd = [mt if p % 2 == 1 else None for p, mt in enumerate(g["mats"])]
    r1 = ctx.cquery(reads, K, M, g["rep"], W, g["N"], even, g["w"], min_class=g["mc"], keep=True)
    try:
        o1 = r1.output()
        same(o1, cr.np_expected_at(col["at"], W, g["N"], even, g["w"], g["mc"]), "even partitions")
        assert not np.array_equal(o1.sums, g["exp"][2])
        o2 = ctx.cquery(reads, K, M, g["rep"], W, g["N"], odd, g["w"], min_class=g["mc"], hits_dev=r1.hits_dev(), sums_dev=r1.sums_dev())
        same(o2, g["exp"], "groups")
        same(r1.output(), g["exp"], "groups, the first result")
    finally:
        r1.free()


def test_device_resident(ctx, col, groups):
    import torch
    from kmtricks_amd import lib
    g = groups
    out = ctx.cquery(col["reads"], K, M, g["rep"], W, g["N"], g["mats"], g["w"], min_class=g["mc"])
    same(out, g["exp"], "host")
    nb = (g["N"] * g["w"] + 7) // 8
    assert out.algo_bytes == sum(len(s) for s in col["reads"]) + int(g["exp"][0].sum(dtype=np.uint64)) * nb + 12 * len(col["reads"]) * g["N"]
    blob, offs = lib.Context.pack_reads(col["reads"])
    dev = torch.device("cuda:0")
    d_b = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_r = torch.from_numpy(g["rep"].view(np.int16)).to(dev)
    d_m = [torch.from_numpy(mt).to(dev) for mt in g["mats"]]
    torch.cuda.synchronize()
    out = ctx.cquery_dev(d_b.data_ptr(), d_o.data_ptr(), len(offs) - 1, K, M, d_r.data_ptr(), W, g["N"], [t.data_ptr() for t in d_m], g["w"], min_class=g["mc"])
    same(out, g["exp"], "device-resident")


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    INVAL, UNSUP = r"\(-2\)", r"\(-5\)"
    rep = orc.repart_static(10, 1)
    body = lambda w: np.zeros((64, w), np.uint8)      # 64 rows of 8 fields
    seq = ["ACGT" * 20]

    def call(code, k=31, m=10, Wn=64, w=4, mc=1, **kw):
        with pytest.raises(lib.KmxError, match=code):
            ctx.cquery(seq, k, m, rep, Wn, 8, [body(w) if 1 <= w <= 8 and Wn == 64 else None], w, min_class=mc, **kw)

    call(INVAL, w=0); call(UNSUP, w=9); call(INVAL, w=33); call(UNSUP, w=32)
    call(INVAL, mc=0); call(INVAL, mc=16); call(INVAL, w=8, mc=256)
    call(INVAL, k=7); call(INVAL, k=128); call(INVAL, m=3); call(UNSUP, Wn=2 ** 32)      # the query section's
    r = ctx.cquery(seq, 31, 10, rep, 64, 8, [body(4)], 4, keep=True)
    try:
        call(INVAL, hits_dev=r.hits_dev()); call(INVAL, sums_dev=r.sums_dev())      # one table without the other
        out = ctx.cquery(seq, 31, 10, rep, 64, 8, [body(4)], 4, hits_dev=r.hits_dev(), sums_dev=r.sums_dev())      # ... both: accepted
        assert out.n_kmers[0] == 50 and not out.hits.any()
    finally:
        r.free()
    # 2^31 queries, 2^32 bases, 2^61 cells: refused from the numbers alone
    offs = np.array([0, 2 ** 32], np.uint64)
    b4 = body(4)
    rows = (C.c_void_p * 1)(b4.ctypes.data)
    for n_seqs, n_cols in ((2 ** 31, 8), (1, 8), (2 ** 30, 2 ** 31)):
        t = lib.KmxCqueryTask(b4.ctypes.data, offs.ctypes.data, n_seqs, 31, 10, rep.ctypes.data, 1, n_cols, 64, rows, 4, 1, None, None)
        res = C.c_void_p()
        assert lib._lib.kmx_cquery_host(ctx._h, C.byref(t), C.byref(res)) == -5 and not res.value
    # and the calls with the one fault mended run
    for w, mc in ((1, 1), (8, 255), (4, 15)):
        out = ctx.cquery(seq, 31, 10, rep, 64, 8, [body(w)], w, min_class=mc)
        assert out.n_kmers[0] == 50 and not out.hits.any() and not out.sums.any()
    out = ctx.cquery(seq, 8, 4, orc.repart_static(4, 1), 2 ** 32 - 1, 8, [None], 4)
    assert out.n_kmers[0] == 73
    out = ctx.cquery(seq, 127, 10, rep, 64, 8, [body(4)], 4)
    assert out.n_kmers[0] == 0


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    """`kmx pipeline --hard-min 1 --bloom-size 4000000` over the two golden samples with the fixture's repartition table, in
    hash:bfc:bin --bitw 4, hash:count:bin and hash:bf:bin"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxcquery")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart", "--bloom-size", 4000000]
    for name, mode in (("bfc", "hash:bfc:bin"), ("count", "hash:count:bin"), ("bf", "hash:bf:bin")):
        r = kmx(*base, "--run-dir", d / name, "--mode", mode, "--bitw", 4)
        assert r.returncode == 0, r.stderr
    hi = open(d / "bfc" / "hash.info", "rb").read()
    Pn, Wn = struct.unpack_from("<QQ", hi, 8)
    assert Pn == 4 and struct.unpack_from("<QQ", open(d / "count" / "hash.info", "rb").read(), 8) == (Pn, Wn)
    mats = []
    for p in range(Pn):
        raw = open(d / "bfc" / "matrices" / f"matrix_{p}.cmbf", "rb").read()
        assert struct.unpack_from("<I", raw, 21)[0] == 8 and len(raw) == 49 + Wn      # two fields of four bits: a byte a row
        mats.append(np.frombuffer(raw[49:], np.uint8).reshape(Wn, 1))
    return dict(dir=d, run=d / "bfc", count=d / "count", bf=d / "bf", W=Wn, mats=mats, rep=t)


@pytest.fixture(scope="module")
def golden_expected(golden_run):
    out = {}
    for s in (1, 2):
        recs = qr.read_fasta_named(os.path.join(GD, f"{s}.fasta"))
        seqs = [r[1] for r in recs]
        at = cr.np_addresses(seqs, 31, 10, golden_run["rep"], golden_run["W"], 4)
        out[s] = dict(names=[r[0] for r in recs], seqs=seqs, **{f"mc{mc}": cr.np_expected_at(at, golden_run["W"], 2, golden_run["mats"], 4, mc) for mc in (1, 2)})
    return out


@pytest.mark.parametrize("sample", [1, 2])
def test_driver_matches_the_restatement(golden_run, golden_expected, sample, tmp_path):
    e = golden_expected[sample]
    names, (n, h, s) = e["names"], e["mc1"]
    run, q = golden_run["run"], os.path.join(GD, f"{sample}.fasta")
    r = kmx("query", "--index", run, "--query", q)
    assert r.returncode == 0, r.stderr
    assert r.stdout == qr.format_matrix(names, ["D1", "D2"], n, h)
    # no false negatives: every k-mer of a sample's own reads has a class of at least 1 in the sample's column
    rows = [line.split("\t") for line in r.stdout.splitlines()[1:]]
    assert len(rows) == len(names) and sum(int(x[1]) for x in rows) > 0
    assert all(x[1] == x[1 + sample] for x in rows)
    for T in (None, 0.0, 1.0):
        r = kmx("query", "--index", run, "--query", q, "--format", "list", "--output", tmp_path / "l.txt", *(() if T is None else ("--threshold", T)))
        assert r.returncode == 0, r.stderr
        assert open(tmp_path / "l.txt").read() == qr.format_list(names, ["D1", "D2"], n, h, 0.7 if T is None else T)
    r = kmx("query", "--index", run, "--query", q, "--format", "sums")
    assert r.returncode == 0, r.stderr
    assert r.stdout == cr.format_sums(names, ["D1", "D2"], n, s)
    n2, h2, s2 = e["mc2"]
    assert not np.array_equal(h, h2) and np.array_equal(s, s2)
    r = kmx("query", "--index", run, "--query", q, "--min-class", 2)
    assert r.returncode == 0 and r.stdout == qr.format_matrix(names, ["D1", "D2"], n2, h2), r.stderr
    r = kmx("query", "--index", run, "--query", q, "--min-class", 2, "--format", "sums")
    assert r.returncode == 0 and r.stdout == cr.format_sums(names, ["D1", "D2"], n, s), r.stderr


def test_driver_groups_and_shards(golden_run, golden_expected):
    """several partition groups (--query-batch-mb), two shards on one device (--gpus 2): the same text"""
    e = golden_expected[1]
    n, h, s = e["mc1"]
    q = os.path.join(GD, "1.fasta")
    for fmt, want in (("matrix", qr.format_matrix(e["names"], ["D1", "D2"], n, h)), ("sums", cr.format_sums(e["names"], ["D1", "D2"], n, s))):
        r = kmx("query", "--index", golden_run["run"], "--query", q, "--format", fmt, "--query-batch-mb", 1, "-v")
        assert r.returncode == 0, r.stderr
        assert r.stdout == want
        mt = re.search(r"(\d+) partition groups a shard", r.stderr)
        assert mt and int(mt.group(1)) >= 3, r.stderr
        r = kmx("query", "--index", golden_run["run"], "--query", q, "--format", fmt, "--gpus", 2, "--query-batch-mb", 1)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        r = kmx("query", "--index", golden_run["run"], "--query", q, "--format", fmt, "--gpus", 2)
        assert r.returncode == 0 and r.stdout == want, r.stderr


def test_driver_agrees_with_the_count_run(golden_run, golden_expected):
    """without the .cmbf: the same samples as a hash:count:bin run -- the sums are floor_of(min(bit_length(count), 15)) of the
    .count_hash row whose hash is h + W * p, added over the query's positions"""
    Wn, rep = golden_run["W"], golden_run["rep"]
    lut = orc.minimizer_lut(10)
    table = {}
    for p in range(4):
        raw = open(golden_run["count"] / "matrices" / f"matrix_{p}.count_hash", "rb").read()[37:]
        assert len(raw) % 16 == 0
        rows = np.frombuffer(raw, np.dtype([("hash", "<u8"), ("c", "<u4", (2,))]))
        assert len(rows) and int(rows["hash"].min()) >= Wn * p and int(rows["hash"].max()) < Wn * (p + 1)
        for hsh, c in zip(rows["hash"].tolist(), rows["c"].tolist()):
            table[hsh] = c
    for sample in (1, 2):
        e = golden_expected[sample]
        sums = np.zeros((len(e["seqs"]), 2), np.uint64)
        memo = {}
        for qi, sq in enumerate(e["seqs"]):
            sq = sq.upper()
            acc = [0, 0]
            for j in range(len(sq) - 31 + 1):
                kmer = sq[j:j + 31]
                if any(ch not in "ACGT" for ch in kmer):
                    continue
                if kmer not in memo:
                    p, h = qr.kmer_address(kmer, 31, 10, lut, rep, Wn)
                    memo[kmer] = table.get(h + Wn * p, (0, 0))
                for i in (0, 1):
                    acc[i] += cr.floor_of(min(int(memo[kmer][i]).bit_length(), 15))
            sums[qi] = acc
        r = kmx("query", "--index", golden_run["run"], "--query", os.path.join(GD, f"{sample}.fasta"), "--format", "sums")
        assert r.returncode == 0, r.stderr
        assert r.stdout == cr.format_sums(e["names"], ["D1", "D2"], e["mc1"][0], sums)
        assert sums.any()


def test_driver_refusals(golden_run, tmp_path):
    q = os.path.join(GD, "1.fasta")
    run, bf = golden_run["run"], golden_run["bf"]

    def refused(*args, word=None):
        r = kmx("query", *args, "--query", q)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
        assert word is None or word in r.stderr, (args, r.stderr)

    refused("--index", run, "--z", 3, word="counting Bloom")
    refused("--index", run, "--min-class", 16, word="--min-class")
    refused("--index", run, "--min-class", 0, word="--min-class")
    refused("--index", bf, "--min-class", 1, word="--min-class")
    refused("--index", bf, "--format", "sums", word="sums")
    refused("--index", golden_run["count"], word="hash:bf:bin")
    shutil.copytree(run, tmp_path / "bits")
    with open(tmp_path / "bits" / "matrices" / "matrix_1.cmbf", "r+b") as f:
        f.seek(21); f.write(struct.pack("<I", 2))
    refused("--index", tmp_path / "bits", word="matrix_1.cmbf")
    shutil.copytree(run, tmp_path / "cut")
    with open(tmp_path / "cut" / "matrices" / "matrix_2.cmbf", "r+b") as f:
        f.truncate(os.path.getsize(tmp_path / "cut" / "matrices" / "matrix_2.cmbf") - 3)
    refused("--index", tmp_path / "cut", word="matrix_2.cmbf")
    shutil.copytree(run, tmp_path / "wide")
    opt = open(tmp_path / "wide" / "options.txt").read()
    assert "bwidth=4" in opt
    with open(tmp_path / "wide" / "options.txt", "w") as f:
        f.write(opt.replace("bwidth=4", "bwidth=12"))
    refused("--index", tmp_path / "wide", word="--bitw")
    r = kmx("query", "--index", run, "--query", q, "--min-class", 15)      # the greatest class of --bitw 4 is accepted
    assert r.returncode == 0, r.stderr
