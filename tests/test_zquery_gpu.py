"""`kmx query --z` on the MI355X against tests/zquery_ref.py (the definition restated with Python integers, and by another road with
numpy): the C ABI through kmtricks_amd.lib on synthetic indexes -- exact equality of n_kmers and hits --, and the driver on the
golden samples.  The indexes are filled to 0.8, so that the AND of four rows still leaves about 0.4 of the bits: any sparser and
wrong zeros and right zeros look alike.  Run with -m gpu."""
import os, re, struct, subprocess
import numpy as np
import pytest

import orc
import query_ref as qr
import zquery_ref as zr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
FILL = 0.8


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, en, eh, what):
    assert np.array_equal(out.n_kmers, en), f"{what}: n_kmers differ at queries {np.nonzero(out.n_kmers != en)[0][:8]}: got {out.n_kmers[out.n_kmers != en][:8]}, expected {en[out.n_kmers != en][:8]}"
    bad = np.argwhere(out.hits != eh)
    assert not len(bad), f"{what}: hits differ in {len(bad)} cells, first (query, sample) {bad[:4].tolist()}: got {[int(out.hits[tuple(b)]) for b in bad[:4]]}, expected {[int(eh[tuple(b)]) for b in bad[:4]]}"


def check(ctx, seqs, k, z, m, rep, W, N, mats, what="", addr=None):
    """the call against the Python-integer road, or with addr (zquery_ref.addresses_np of the same inputs) the numpy road"""
    if addr is None:
        en, eh = zr.zquery_expected(seqs, k, z, m, rep, W, N, mats)
    else:
        en, eh = zr.zquery_expected_np(seqs, k, z, m, rep, W, N, mats, addr=addr)
    out = ctx.zquery(seqs, k, m, rep, W, N, mats, z)
    same(out, en, eh, what)
    return out


@pytest.fixture(scope="module")
def column_case():
    reads = qr.random_reads(5, 60, 150)
    return reads, zr.addresses_np(reads, 31, 10, orc.repart_static(10, 4), 4099)


@pytest.mark.parametrize("N", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 513, 2049, 2500])
def test_columns(ctx, column_case, N):
    """every width of a row around the byte, dword, 64-dword and second-pass edges of the row fetch and the window pass, and the
    padding of the table's pitch; every padding bit of every row is 1 in the input"""
    reads, addr = column_case
    mats, rep = qr.synth_index(100 + N, N, 4099, 4, 31, 10, FILL, pad_ones=True)
    if N % 8:
        assert all((mt[:, -1] >> (N % 8)).min() == (0xFF >> (N % 8)) for mt in mats)
    out = check(ctx, reads, 31, 3, 10, rep, 4099, N, mats, f"N={N}", addr=addr)
    assert (out.n_kmers == 150 - 34 + 1).all() and 0.2 < out.hits.mean() / 117 < 0.6      # FILL ** 4 = 0.41


@pytest.mark.parametrize("z", [0, 1, 2, 3, 7, 8])
def test_window_lengths(ctx, z):
    k, m, W, N, P = 31, 10, 10007, 65, 8
    mats, rep = qr.synth_index(40 + z, N, W, P, k, m, FILL, pad_ones=True)
    reads = qr.random_reads(z, 40, 150) + qr.random_reads(z + 1, 2, 700)
    out = check(ctx, reads, k, z, m, rep, W, N, mats, f"z={z}")
    if z == 0:      # by definition the plain query's result, array for array
        plain = ctx.query(reads, k, m, rep, W, N, mats)
        assert np.array_equal(out.n_kmers, plain.n_kmers) and np.array_equal(out.hits, plain.hits)


@pytest.mark.parametrize("k", [12, 21, 31, 32, 33, 63, 64, 96, 127])
def test_kmer_sizes(ctx, k):
    m = 8 if k == 12 else 10
    mats, rep = qr.synth_index(k, 65, 10007, 8, k, m, FILL, pad_ones=True)
    reads = qr.random_reads(k, 40, 150) + qr.random_reads(k + 1, 2, 700)
    check(ctx, reads, k, 3, m, rep, 10007, 65, mats, f"k={k}")


def test_query_shapes(ctx):
    k, z, m, W, N, P = 31, 3, 10, 4099, 65, 4
    K = k + z
    mats, rep = qr.synth_index(9, N, W, P, k, m, FILL, pad_ones=True)
    rnd = lambda seed, n: qr.random_reads(seed, 1, n)[0]
    unit = rnd(20, 30)
    seqs = ["", rnd(1, k - 1), rnd(2, K - 1), rnd(3, K), rnd(4, K + 1),                     # K - 1 bases: four k-mers, no K-position
            rnd(5, 63 + K - 1), rnd(6, 64 + K - 1), rnd(7, 65 + K - 1),                    # 63, 64, 65 K-positions: the item's edge
            rnd(8, 126 + K - 1), rnd(9, 127 + K - 1),                                      # 126, 127: two items
            "N" + rnd(10, 99), rnd(11, 99) + "N", "N".join(rnd(30 + i, K - 1) for i in range(6)),      # an N at base 0, at the last base, at every K-th base
            rnd(12, 50) + "N" + rnd(13, 50),      # k-mers at 0 .. 19 and 51 .. 70; the windows at 17 .. 19 reach over the N
            rnd(14, k) + "N" + rnd(15, k),        # a k-mer on either side of the N, no window anywhere
            rnd(16, 200).lower(), "A" * 120, (unit * 10)[:300], "", rnd(17, 5)]
    out = check(ctx, seqs, k, z, m, rep, W, N, mats, "shapes")
    assert list(out.n_kmers) == [0, 0, 0, 1, 2, 63, 64, 65, 126, 127, 66, 66, 0, 34, 0, 167, 87, 267, 0, 0]
    assert not out.hits[[0, 1, 2, 12, 14, 18, 19]].any()
    # a homopolymer's k-mers are one k-mer: every window has that row
    assert set(out.hits[16].tolist()) <= {0, 87} and 87 in out.hits[16]


@pytest.fixture(scope="module")
def ones_index():
    """every byte 0xFF: N = 9 columns in rows of two bytes, two partitions of 257 rows"""
    return [np.full((257, 2), 0xFF, np.uint8) for _ in range(2)], orc.repart_static(10, 2)


def test_no_leak_across_queries(ctx, ones_index):
    """an all-ones index: hits[q][i] == n_kmers[q] == len - K + 1 for every query.  A window that reaches into a neighbour, or an item
    that flushes to the wrong query, breaks the equality"""
    k, z, N = 31, 3, 9
    K = k + z
    mats, rep = ones_index
    seqs = []
    for i in range(200):
        seqs.append(qr.random_reads(1000 + i, 1, K + i * 37 % 71)[0])      # every length from K to K + 70
        if i % 7 == 0:
            seqs.append("")
        if i % 31 == 0:
            seqs += ["", ""]
    out = ctx.zquery(seqs, k, 10, rep, 257, N, mats, z)
    want = np.array([max(0, len(s) - K + 1) for s in seqs], np.uint32)
    assert (want == 0).sum() > 30 and want.max() == 71 and want[want > 0].min() == 1
    assert np.array_equal(out.n_kmers, want)
    assert np.array_equal(out.hits, np.repeat(want[:, None], N, axis=1))


def test_counter_width(ctx, ones_index):
    """one 70 000-base query against the all-ones index: sums far past 65 535"""
    mats, rep = ones_index
    seq = qr.random_reads(77, 1, 70000)
    out = ctx.zquery(seq, 31, 10, rep, 257, 9, mats, 3)
    n = 70000 - 34 + 1
    assert out.n_kmers[0] == n > 65535 and (out.hits[0] == n).all()


@pytest.fixture(scope="module")
def group_case():
    k, z, m, W, N, P = 31, 3, 10, 4099, 65, 8
    mats, rep = qr.synth_index(61, N, W, P, k, m, FILL, pad_ones=True)
    reads = qr.random_reads(62, 60, 150)
    addr = zr.addresses_np(reads, k, m, rep, W)
    groups = [[0, 3, 6], [1, 4, 7], [2, 5]]
    only = lambda g: [mt if p in g else None for p, mt in enumerate(mats)]
    return dict(k=k, z=z, m=m, W=W, N=N, mats=mats, rep=rep, reads=reads, addr=addr, parts=[only(g) for g in groups], only=only)


def series(ctx, c, parts, hits_dev=None, keep=False):
    """the calls of one series: the first one's kept result owns the table, the last one has `last`"""
    args = (c["reads"], c["k"], c["m"], c["rep"], c["W"], c["N"])
    first = ctx.zquery(*args, parts[0], c["z"], last=len(parts) == 1, hits_dev=hits_dev, keep=True)
    if len(parts) == 1:
        return first, first
    try:
        for mm in parts[1:-1]:
            assert ctx.zquery(*args, mm, c["z"], bits_dev=first.bits_dev(), last=False) is None
        return first, ctx.zquery(*args, parts[-1], c["z"], bits_dev=first.bits_dev(), hits_dev=hits_dev, last=True, keep=keep)
    except Exception:
        first.free()
        raise


def test_partition_groups(ctx, group_case):
    """eight partitions dealt into three groups, three calls sharing the first call's table: the one-call result"""
    from kmtricks_amd import lib
    c = group_case
    en, eh = zr.zquery_expected_np(c["reads"], c["k"], c["z"], c["m"], c["rep"], c["W"], c["N"], c["mats"], addr=c["addr"])
    one = ctx.zquery(c["reads"], c["k"], c["m"], c["rep"], c["W"], c["N"], c["mats"], c["z"])
    same(one, en, eh, "one call")
    first, out = series(ctx, c, c["parts"])
    try:
        same(out, en, eh, "three groups")
        # a result without `last` has no n_kmers and no hits
        assert not first.hits_dev() and first.bits_dev()
        with pytest.raises(lib.KmxError):
            first.output()
    finally:
        first.free()
    # a group that is never sent: the restatement with those matrices None
    first, out = series(ctx, c, [c["parts"][0], c["parts"][2]])
    first.free()
    en2, eh2 = zr.zquery_expected_np(c["reads"], c["k"], c["z"], c["m"], c["rep"], c["W"], c["N"], c["only"]([0, 3, 6, 2, 5]), addr=c["addr"])
    same(out, en2, eh2, "a group never sent")
    assert np.array_equal(en2, en) and (eh2 <= eh).all() and (eh2 < eh).any()
    # a second series adds into the first one's hits table: twice the table
    first, kept = series(ctx, c, c["parts"], keep=True)
    first.free()
    try:
        first2, out2 = series(ctx, c, c["parts"][::-1], hits_dev=kept.hits_dev())
        first2.free()
        same(out2, en, 2 * eh, "a second series into the same table")
        assert np.array_equal(kept.output().hits, 2 * eh)
    finally:
        kept.free()


def test_host_and_device_inputs(ctx):
    """one 200 000-base query beside 2 000 reads of 100 bp, 32 partitions: host and device-resident inputs, the bytes of the call"""
    import torch
    from kmtricks_amd import lib
    k, z, m, W, N, P = 31, 3, 10, 65521, 100, 32
    mats, rep = qr.synth_index(21, N, W, P, k, m, FILL, pad_ones=True)
    seqs = qr.random_reads(22, 1, 200_000) + qr.random_reads(23, 2000, 100)
    en, eh = zr.zquery_expected_np(seqs, k, z, m, rep, W, N, mats)
    out = ctx.zquery(seqs, k, m, rep, W, N, mats, z)
    same(out, en, eh, "host inputs")
    # all bases ACGT: every query has len - k + 1 k-mers, all of partitions that are part of the call; nb = 13, pitch = 16
    found = sum(len(s) - k + 1 for s in seqs)
    assert out.algo_bytes == sum(len(s) for s in seqs) + found * (13 + 16) + (int(en.sum(dtype=np.uint64)) + z * len(seqs)) * 16 + 4 * len(seqs) * N
    blob, offs = lib.Context.pack_reads(seqs)
    dev = torch.device("cuda:0")
    d_b = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_r = torch.from_numpy(rep.view(np.int16)).to(dev)
    d_m = [torch.from_numpy(mt).to(dev) for mt in mats]
    torch.cuda.synchronize()
    out = ctx.zquery_dev(d_b.data_ptr(), d_o.data_ptr(), len(offs) - 1, k, m, d_r.data_ptr(), W, N, [t.data_ptr() for t in d_m], z)
    same(out, en, eh, "device inputs")


@pytest.mark.parametrize("W,P", [(1, 1), (255, 256), (2 ** 20 + 7, 1)])
def test_window_edges(ctx, W, P):
    k, z, m, N = 31, 3, 10, 9
    mats, rep = qr.synth_index(W % 1000 + P, N, W, P, k, m, FILL, pad_ones=True)
    assert P == 1 or int(rep.max()) == P - 1
    check(ctx, qr.random_reads(W % 97 + P, 60, 120), k, z, m, rep, W, N, mats, f"W={W} P={P}")


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    for kw in (dict(z=9), dict(k=8, m=4, z=8), dict(k=7), dict(k=128), dict(m=3), dict(W=2 ** 32)):
        rep = orc.repart_static(kw.get("m", 10), 1)
        with pytest.raises(lib.KmxError):
            ctx.zquery(["ACGT" * 20], kw.get("k", 31), kw.get("m", 10), rep, kw.get("W", 64), 8, [None], kw.get("z", 3))
    # (the same calls with their one fault mended are accepted)
    out = ctx.zquery(["ACGT" * 20], 8, 4, orc.repart_static(4, 1), 64, 8, [None], 7)
    assert out.n_kmers[0] == 80 - 15 + 1 and not out.hits.any()


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    """`kmx pipeline --mode hash:bf:bin --hard-min 1` over the two golden samples, with the fixture's repartition table"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxzquery")
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
        n, h = zr.zquery_expected([r[1] for r in recs], 31, 3, 10, golden_run["rep"], golden_run["W"], 2, golden_run["mats"])
        out[s] = ([r[0] for r in recs], n, h)
    return out


@pytest.mark.parametrize("sample", [1, 2])
def test_driver_matches_the_restatement(golden_run, golden_expected, sample, tmp_path):
    names, n, h = golden_expected[sample]
    q = os.path.join(GD, f"{sample}.fasta")
    r = kmx("query", "--index", golden_run["run"], "--query", q, "--z", 3)
    assert r.returncode == 0, r.stderr
    assert r.stdout == qr.format_matrix(names, ["D1", "D2"], n, h)
    # no false negatives: every K-mer of a sample's own reads is in the sample's column
    rows = [line.split("\t") for line in r.stdout.splitlines()[1:]]
    assert len(rows) == len(names) and sum(int(x[1]) for x in rows) > 0
    assert all(x[1] == x[1 + sample] for x in rows)
    for T in (None, 1.0):
        r = kmx("query", "--index", golden_run["run"], "--query", q, "--z", 3, "--format", "list", "--output", tmp_path / "l.txt", *(() if T is None else ("--threshold", T)))
        assert r.returncode == 0, r.stderr
        assert open(tmp_path / "l.txt").read() == qr.format_list(names, ["D1", "D2"], n, h, 0.7 if T is None else T)


def test_driver_z_zero_and_groups(golden_run, golden_expected):
    """--z 0 is the text of a run without --z, byte for byte; several partition groups and query batches give the same text"""
    q = os.path.join(GD, "1.fasta")
    plain = kmx("query", "--index", golden_run["run"], "--query", q)
    r = kmx("query", "--index", golden_run["run"], "--query", q, "--z", 0)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr + r.stderr
    assert r.stdout == plain.stdout and len(plain.stdout.splitlines()) > 1
    names, n, h = golden_expected[1]
    r = kmx("query", "--index", golden_run["run"], "--query", q, "--z", 3, "--query-batch-mb", 1, "-v")
    assert r.returncode == 0, r.stderr
    assert r.stdout == qr.format_matrix(names, ["D1", "D2"], n, h)
    mt = re.search(r"(\d+) partition groups a shard", r.stderr)
    assert mt and int(mt.group(1)) >= 3, r.stderr


def test_driver_refusals(golden_run, tmp_path):
    q = os.path.join(GD, "1.fasta")
    # an index whose options.txt says k = 8: the only k at which a Z of at most 8 is not below it
    os.makedirs(tmp_path / "k8")
    open(tmp_path / "k8" / "kmtricks.fof", "w").write(open(golden_run["run"] / "kmtricks.fof").read())
    opt = open(golden_run["run"] / "options.txt").read()
    assert "kmer_size=31" in opt
    open(tmp_path / "k8" / "options.txt", "w").write(opt.replace("kmer_size=31", "kmer_size=8"))
    for index, run, extra, word in (("--index", golden_run["run"], ("--z", 9), "[0, 8]"), ("--index", golden_run["run"], ("--z", -1), "[0, 8]"),
                                    ("--index", tmp_path / "k8", ("--z", 8), "k-mer size"),
                                    ("--kmer-index", golden_run["run"], ("--z", 3), "--kmer-index"),
                                    ("--index", golden_run["run"], ("--z", 3, "--gpus", 2), "--gpus")):
        r = kmx("query", index, run, "--query", q, *extra)
        assert r.returncode == 1 and "[error]" in r.stderr and word in r.stderr and r.stdout == "", (extra, r.returncode, r.stderr)
