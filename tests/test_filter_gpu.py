"""`kmx filter` on the MI355X, byte for byte against tests/filter_ref.py (the definition restated with a dictionary and a set): the
C ABI (kmx_filter_host / kmx_filter_dev through kmtricks_amd.lib) on synthetic matrices over the whole key space, a partition in runs
of rows with the marks carried over, device-resident inputs, the driver on the golden samples, and a property that needs no
restatement.  Run with -m gpu."""
import itertools, os, subprocess, sys
import numpy as np
import pytest

import filter_ref as fr
from synth import SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def check(ctx, case, n_cols, kw, mode, want="kmv", what=""):
    row_keys, payload, key_keys, key_counts = case
    em, ev, eak, eac = fr.filter_expected(row_keys, payload, key_keys, key_counts, mode)
    out = ctx.filter(fr.matrix_body(row_keys, payload), n_cols, kw, mode, (key_keys, key_counts), want)
    irb = 8 * kw + fr.payload_bytes(n_cols, mode)
    assert out.row_bytes == irb + (4 if mode == fr.MODE_COUNT else 0), what
    assert out.rows == len(em) // out.row_bytes, what
    if "m" in want:
        if out.body != em:
            a, b = np.frombuffer(out.body, np.uint8), np.frombuffer(em, np.uint8)
            bad = np.nonzero(a != b)[0] if len(a) == len(b) else [min(len(a), len(b))]
            raise AssertionError(f"{what}: m has {len(a)} bytes, expected {len(b)}; differs at {len(bad)} bytes, first at {bad[:8]}")
    else:
        assert out.body == b"", what
    if "v" in want:
        assert np.array_equal(out.vector, ev), what
    else:
        assert len(out.vector) == 0, what
    if "k" in want:
        assert np.array_equal(out.absent_keys, eak) and np.array_equal(out.absent_counts, eac), what
    else:
        assert len(out.absent_counts) == 0 and len(out.absent_keys) == 0, what


@pytest.mark.parametrize("kw", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_key_shapes(ctx, kw, shape):
    """every key width over the five full-width shapes, count and PA, a share of the rows kept"""
    for mode in (fr.MODE_COUNT, fr.MODE_PA):
        for n_cols, keep in ((7, 0.5), (200, 0.01)):
            case = fr.synth_case(11 * kw + n_cols, 3000, n_cols, kw, mode, keep, 1.0, shape, extreme=True)
            check(ctx, case, n_cols, kw, mode, what=f"{shape} kw={kw} mode={mode} N={n_cols} keep={keep}")


@pytest.mark.parametrize("n_cols", [1, 7, 8, 9, 200, 1000, 4096])
@pytest.mark.parametrize("mode", [fr.MODE_COUNT, fr.MODE_PA])
def test_columns_and_share_kept(ctx, n_cols, mode):
    """N from 1 to 4096 (a 16 KB row); none, about 1 %, about half and all of the rows kept"""
    n_rows = 2000 if n_cols <= 200 else 600
    for kw, keep in itertools.product((1, 2), (0.0, 0.01, 0.5, 1.0)):
        case = fr.synth_case(n_cols + 17 * kw, n_rows, n_cols, kw, mode, keep, 1.0, "uniform", extreme=(keep == 0.5))
        check(ctx, case, n_cols, kw, mode, what=f"N={n_cols} mode={mode} kw={kw} keep={keep}")


@pytest.mark.parametrize("mode", [fr.MODE_COUNT, fr.MODE_PA])
@pytest.mark.parametrize("ratio,keep", [(10.0, 0.5), (10.0, 1.0), (0.1, 0.05), (0.1, 0.0)])
def test_key_denser_and_sparser_than_the_rows(ctx, mode, ratio, keep):
    """a key list ten times as long as the matrix (a tile's span of it does not fit the LDS: the rows search global memory) and
    ten times shorter"""
    for kw in (1, 3):
        case = fr.synth_case(5, 4000, 9, kw, mode, keep, ratio)
        check(ctx, case, 9, kw, mode, what=f"ratio={ratio} keep={keep} kw={kw} mode={mode}")


def hand_cases():
    """(name, kw, row keys, key keys): the edge cases of test_filter_cpu.py"""
    K = lambda *v: np.array(v, np.uint64).reshape(len(v), -1)
    b63 = 1 << 63
    yield "worked example", 1, K(3, 5, 9, 12), K(1, 5, 9, 20)
    yield "empty key", 1, K(3, 5, 9), np.zeros((0, 1), np.uint64)
    yield "empty matrix", 1, np.zeros((0, 1), np.uint64), K(3, 5)
    yield "key below the first row", 1, K(100, 200, 300), K(1, 2, 99)
    yield "key above the last row", 1, K(100, 200, 300), K(301, 5000, 2 ** 64 - 1)
    yield "key = rows", 1, K(0, 1, b63 - 1, b63, 2 ** 64 - 1), K(0, 1, b63 - 1, b63, 2 ** 64 - 1)
    yield "one row kept", 1, K(42), K(42)
    yield "one row dropped", 1, K(42), K(41, 43)
    yield "bit 63 of the low word", 1, K(5, 5 | b63), K(5 | b63)
    for kw in (2, 3, 4):
        top = [0] * (kw - 1)
        yield f"bit 63 of the low word, {kw} words", kw, K([5] + top, [5 | b63] + top), K([5 | b63] + top)
        yield f"the top word alone, {kw} words", kw, K([7] * (kw - 1) + [1], [7] * (kw - 1) + [b63], [7] * (kw - 1) + [b63 + 1]), K([7] * (kw - 1) + [b63], [7] * (kw - 1) + [2])


@pytest.mark.parametrize("mode", [fr.MODE_COUNT, fr.MODE_PA])
def test_edge_cases(ctx, mode):
    rng = np.random.default_rng(3)
    for name, kw, rows, key in hand_cases():
        rows, key = fr.sort_keys(rows) if len(rows) else rows.reshape(0, kw), fr.sort_keys(key) if len(key) else key.reshape(0, kw)
        for n_cols in (1, 9):
            payload = rng.integers(0, 256, (len(rows), fr.payload_bytes(n_cols, mode)), dtype=np.uint8)
            counts = rng.integers(1, 2 ** 32, len(key), dtype=np.uint64).astype(np.uint32)
            check(ctx, (rows, payload, key, counts), n_cols, kw, mode, what=f"{name} mode={mode} N={n_cols}")


@pytest.mark.parametrize("mode", [fr.MODE_COUNT, fr.MODE_PA])
def test_many_tiles(ctx, mode):
    """300 000 rows: more than a thousand tiles, placed by the scan across workgroups"""
    check(ctx, fr.synth_case(9, 300000, 3, 1, mode, 0.5), 3, 1, mode, what="300000 rows")


def test_headline_rows(ctx):
    """20 000 rows of 1000 u32 columns"""
    check(ctx, fr.synth_case(21, 20000, 1000, 1, fr.MODE_COUNT, 0.5), 1000, 1, fr.MODE_COUNT, what="20000 x 1000")


def test_rows_above_64_kb(ctx):
    """16 500 count columns: a row of 66 008 bytes, two of which are more than the 128 KB a workgroup of k_filter_move takes -- it
    moves one row (sr = 1), the tile's 256 ranks one by one"""
    n_cols = 16500
    irb, sr = 8 + 4 * n_cols, 256
    while sr > 1 and sr * irb > 131072:      # launch_filter_move (kmtricks_amd/csrc/filter.hip)
        sr >>= 1
    assert sr == 1 and irb > 65536
    check(ctx, fr.synth_case(165, 100, n_cols, 1, fr.MODE_COUNT, 0.5, extreme=True), n_cols, 1, fr.MODE_COUNT, what="100 x 16500")


@pytest.mark.parametrize("want", ["k", "m", "v", "km", "kv", "mv", "kmv"])
def test_every_subset_of_outputs(ctx, want):
    for mode in (fr.MODE_COUNT, fr.MODE_PA):
        check(ctx, fr.synth_case(2, 3000, 12, 2, mode, 0.3), 12, 2, mode, want, what=f"want={want} mode={mode}")


@pytest.mark.parametrize("mode", [fr.MODE_COUNT, fr.MODE_PA])
@pytest.mark.parametrize("run", [1, 2, 1000])
def test_runs_of_rows_with_the_marks_carried_over(ctx, mode, run):
    """the partition in one call and in runs of `run` rows: m and v concatenate, k comes out of the last run"""
    n_rows, n_cols, kw = (40 if run <= 2 else 3500), 5, 2
    row_keys, payload, key_keys, key_counts = fr.synth_case(77, n_rows, n_cols, kw, mode, 0.5, 2.0)
    whole = ctx.filter(fr.matrix_body(row_keys, payload), n_cols, kw, mode, (key_keys, key_counts), "kmv")
    em, ev, eak, eac = fr.filter_expected(row_keys, payload, key_keys, key_counts, mode)
    assert whole.body == em and np.array_equal(whole.vector, ev) and np.array_equal(whole.absent_keys, eak)
    marks = np.zeros(len(key_counts), np.uint8)
    bodies, vecs, last = [], [], None
    starts = list(range(0, len(row_keys), run))
    for s in starts:
        final = s == starts[-1]
        last = ctx.filter(fr.matrix_body(row_keys[s:s + run], payload[s:s + run]), n_cols, kw, mode, (key_keys, key_counts),
                          "kmv" if final else "mv", marks=marks)
        bodies.append(last.body); vecs.append(last.vector)
    assert b"".join(bodies) == whole.body
    assert np.array_equal(np.concatenate(vecs), whole.vector)
    assert np.array_equal(last.absent_keys, whole.absent_keys) and np.array_equal(last.absent_counts, whole.absent_counts)
    assert int(marks.sum()) == whole.rows


def test_refusals(ctx):
    from kmtricks_amd import lib
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        with pytest.raises(lib.KmxError, match=r"\(-5\).*Bloom"):
            ctx.filter_dev(None, 0, 2, 1, mode, (None, 0), "m")
    with pytest.raises(lib.KmxError, match=r"\(-2\).*mode"):
        ctx.filter_dev(None, 0, 2, 1, 9, (None, 0), "m")
    with pytest.raises(lib.KmxError, match=r"\(-2\).*key_words"):
        ctx.filter_dev(None, 0, 2, 5, lib.MODE_COUNT, (None, 0), "m")
    with pytest.raises(lib.KmxError, match=r"\(-2\).*want"):
        ctx.filter_dev(None, 0, 2, 1, lib.MODE_COUNT, (None, 0), 0)
    with pytest.raises(lib.KmxError, match=r"\(-2\).*column"):
        ctx.filter_dev(None, 0, 0, 1, lib.MODE_COUNT, (None, 0), "m")


def test_device_resident_inputs(ctx):
    """the key list straight from count_reads_dev, the rows straight from MergeResult.body_dev of a file-order merge: nothing comes to
    the host in between"""
    import orc
    from kmtricks_amd import lib
    rng = np.random.default_rng(5)
    genome = "".join(rng.choice(list("ACGT"), size=6000))
    def reads(seed, n):
        r = np.random.default_rng(seed)
        return [genome[a:a + 120] for a in r.integers(0, len(genome) - 120, n)]
    k, m, P = 31, 10, 4
    lut, rep = orc.minimizer_lut(m), orc.repart_static(m, P)
    store = lib.Store(0)
    try:
        samples = [reads(s, 150) for s in (1, 2, 3)]
        lists = [ctx.count_reads_dev(s, k, m, rep, P, 1, [store])[0] for s in samples]
        key_lists, _, _ = ctx.count_reads_dev(reads(9, 200) + ["".join(rng.choice(list("ACGT"), size=120)) for _ in range(50)], k, m, rep, P, 2, [store])
        for mode in (lib.MODE_COUNT, lib.MODE_PA):
            for p in range(P):
                res = ctx.merge_dev([dict(lists=[l[p] for l in lists], key_words=1, soft_min=[1, 1, 1], rec_min=1, share_min=0, mode=mode)])
                res.wait()
                rows, body_dev = res.rows(), res.body_dev()
                out = ctx.filter_dev(body_dev, rows, 3, 1, mode, key_lists[p], "kmv")
                row_keys, payload = fr.split_body(res.body(), 1, 3, mode)
                kk, kc = ctx.read_list(key_lists[p][0], key_lists[p][1], 1)
                em, ev, eak, eac = fr.filter_expected(row_keys, payload, kk, kc, mode)
                assert rows > 0 and len(kc) > 0 and 0 < (ev != 0).sum() < rows
                assert out.body == em and np.array_equal(out.vector, ev)
                assert np.array_equal(out.absent_keys, eak) and np.array_equal(out.absent_counts, eac)
                res.free()
    finally:
        store.close()


def test_stress_script():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "stress_filter.py"), "--cases", "30", "--seed", "1"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the driver ----------------------------------------------------------------------------------------------------------------
import ctypes, shutil, struct
import kmfiles
from test_oracle_goldens import repart_table, read_fasta, GD

KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
M, P = 10, 4


def unlz4(b):
    lz4 = ctypes.CDLL("liblz4.so.1")
    dctx = ctypes.c_void_p()
    assert lz4.LZ4F_createDecompressionContext(ctypes.byref(dctx), 100) == 0
    lz4.LZ4F_decompress.restype = ctypes.c_size_t
    out = bytearray(); src = ctypes.create_string_buffer(b, len(b)); pos = 0
    while pos < len(b):
        dst = ctypes.create_string_buffer(1 << 16); dn = ctypes.c_size_t(1 << 16); sn = ctypes.c_size_t(len(b) - pos)
        r = lz4.LZ4F_decompress(dctx, dst, ctypes.byref(dn), ctypes.byref(src, pos), ctypes.byref(sn), None)
        assert not lz4.LZ4F_isError(ctypes.c_size_t(r))
        out += dst.raw[:dn.value]; pos += sn.value
        if r == 0 and dn.value == 0 and sn.value == 0: break
    return bytes(out)


def sh(*cmd):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the fixture repartition, the two golden samples as a fof, and a third sample: half of its reads from 1.fasta (each twice, so
    that they pass a hard-min of 2), half random"""
    d = tmp_path_factory.mktemp("kmxfilter")
    t = repart_table()
    (d / "fixture.minimRepart").write_bytes(struct.pack("<HQH", 4, len(t), 1) + t.tobytes() + struct.pack("<BI", 0, 0x12345678))
    (d / "in.fof").write_text(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    rng = np.random.default_rng(12)
    one = read_fasta(os.path.join(GD, "1.fasta"))
    reads = [s for s in one[::2]] * 2 + ["".join(rng.choice(list("ACGT"), size=len(one[0]))) for _ in range(len(one) // 2)] * 2 + one[1::4]
    (d / "key.fasta").write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    (d / "key.fof").write_text(f"Q1 : {d}/key.fasta\n")
    (d / "key_min3.fof").write_text(f"Q1 : {d}/key.fasta ! 3\n")
    return d, reads


def pipeline(inputs, out, mode, k=31, fof=None, *extra):
    sh(KMX, "pipeline", "--file", fof or inputs[0] / "in.fof", "--run-dir", out, "--kmer-size", k, "--hard-min", "1", "--nb-partitions", "4",
       "--repart-file", inputs[0] / "fixture.minimRepart", "--mode", mode, *extra)
    return out


def key_counts(reads, k, hard_min):
    import orc
    sk = orc.superk_partition(reads, k, M, orc.minimizer_lut(M), repart_table(), P)
    return [orc.count_kmer(s[0], k, hard_min) for s in sk]


def read_matrix(path, pa):
    raw = open(path, "rb").read()
    body = unlz4(raw[45:]) if raw[12] else raw[45:]
    return raw[:45], body


def check_run(run_dir, out, pa, reads, k, hard_min, want="mv", cpr_in=False, cpr_out=False, sid="Q1"):
    """the output run `out` of a filter of `run_dir` against filter_ref"""
    kw, ext = (k + 31) // 32, "pa" if pa else "count"
    mode = fr.MODE_PA if pa else fr.MODE_COUNT
    lists = key_counts(reads, k, hard_min)
    for d in ("matrices", "counts", "config_gatb", "repartition_gatb"):
        assert (out / d).is_dir()
    assert (out / "kmtricks.fof").is_file()
    assert open(out / "config_gatb" / "gatb.config", "rb").read() == open(run_dir / "config_gatb" / "gatb.config", "rb").read()
    assert open(out / "repartition_gatb" / "repartition.minimRepart", "rb").read() == open(run_dir / "repartition_gatb" / "repartition.minimRepart", "rb").read()
    kept = 0
    for p in range(P):
        hdr, body = read_matrix(run_dir / "matrices" / f"matrix_{p}.{ext}{'.lz4' if cpr_in else ''}", pa)
        n = struct.unpack_from("<I", hdr, 29 if pa else 33)[0]
        row_keys, payload = fr.split_body(body, kw, n, mode)
        em, ev, eak, eac = fr.filter_expected(row_keys, payload, lists[p][0], lists[p][1], mode)
        kept += len(em)
        mpath = out / "matrices" / f"matrix_{p}.{ext}{'.lz4' if cpr_out else ''}"
        if "m" in want:
            oh, ob = read_matrix(mpath, pa)
            assert oh[12] == (1 if cpr_out else 0) and oh[:12] == hdr[:12] and oh[13:21] == hdr[13:21]
            if pa:
                assert oh[13:] == hdr[13:]                                       # the PA header is unchanged
            else:
                assert struct.unpack_from("<IIIIII", oh, 21) == (k, kw, 1, n + 1, 0, p)
            assert ob == em, f"partition {p}"
        else:
            assert not mpath.exists()
        if "v" in want:
            assert open(out / "matrices" / f"{p}.vec").read() == "".join(f"{int(x)}\n" for x in ev)
        else:
            assert not (out / "matrices" / f"{p}.vec").exists()
        kpath = out / "counts" / f"partition_{p}" / f"{sid}.kmer{'.lz4' if cpr_out else ''}"
        if "k" in want:
            raw = open(kpath, "rb").read()
            assert raw[12] == (1 if cpr_out else 0)
            tmp = out / f"k{p}.kmer"
            tmp.write_bytes(raw[:12] + b"\0" + raw[13:41] + (unlz4(raw[41:]) if cpr_out else raw[41:]))
            f = kmfiles.read_kmer_file(tmp)
            assert (f["k"], f["slots"], f["count_slots"], f["id"], f["partition"]) == (k, kw, 4, 0, p)
            assert np.array_equal(f["keys"], eak) and np.array_equal(f["counts"], eac)
        else:
            assert not kpath.exists()
    return kept


@pytest.mark.parametrize("mode", ["kmer:count:bin", "kmer:pa:bin"])
def test_driver_on_the_golden_samples(inputs, tmp_path, mode):
    pa = "pa" in mode
    run_dir = pipeline(inputs, tmp_path / "run", mode)
    for i, (types, want) in enumerate((("k,m,v", "kmv"), (None, "mv"), ("k", "k"), ("m", "m"), ("v", "v"))):
        out = tmp_path / f"out{i}"
        sh(KMX, "filter", "--in-matrix", run_dir, "--key", inputs[0] / "key.fof", "--output", out, *(["--out-types", types] if types else []))
        kept = check_run(run_dir, out, pa, inputs[1], 31, 2, want)
        assert kept > 0 or "m" not in want
    # a minimum in the fof line beats --hard-min (the smallest batch size too: these matrices are one run each, the several-runs
    # case is test_driver_runs_of_rows)
    out = tmp_path / "out_min3"
    sh(KMX, "filter", "--in-matrix", run_dir, "--key", inputs[0] / "key_min3.fof", "--output", out, "--hard-min", "1", "--out-types", "k,m,v", "--filter-batch-mb", "1")
    check_run(run_dir, out, pa, inputs[1], 31, 3, "kmv")
    assert key_counts(inputs[1], 31, 3)[0][0].shape != key_counts(inputs[1], 31, 1)[0][0].shape


def test_driver_compressed_in_and_out(inputs, tmp_path):
    run_dir = pipeline(inputs, tmp_path / "run", "kmer:count:bin", 31, None, "--cpr")
    out = tmp_path / "out"
    sh(KMX, "filter", "--in-matrix", run_dir, "--key", inputs[0] / "key.fof", "--output", out, "--cpr-in", "--cpr-out", "--out-types", "k,m,v")
    assert check_run(run_dir, out, False, inputs[1], 31, 2, "kmv", cpr_in=True, cpr_out=True) > 0


def test_driver_runs_of_rows(inputs, tmp_path):
    """a matrix of the test's own making, large enough (40 samples, about 100 000 rows a partition) for --filter-batch-mb 1 to cut
    every partition into several runs of rows"""
    rng = np.random.default_rng(4)
    genome = "".join(rng.choice(list("ACGT"), size=400000))
    reads = [genome[i:i + 200] for i in range(0, len(genome) - 200, 150)]
    fa = tmp_path / "big.fasta"; fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    fofs = tmp_path / "big.fof"; fofs.write_text("".join(f"B{i} : {fa}\n" for i in range(40)))      # rows of 8 + 160 bytes, ~100 000 a partition
    run_dir = pipeline(inputs, tmp_path / "run", "kmer:count:bin", 31, fofs)
    key = reads[::3] + ["".join(rng.choice(list("ACGT"), size=200)) for _ in range(300)]
    kf = tmp_path / "k.fasta"; kf.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(key)))
    kfof = tmp_path / "k.fof"; kfof.write_text(f"Q1 : {kf}\n")
    assert os.path.getsize(run_dir / "matrices" / "matrix_0.count") > 4 << 20      # several runs of 1 MB
    # every subset of the outputs in runs of 1 MB (a k-only job still has to leave the marks of every run), then two shards
    for types in ("k", "m", "v", "k,m", "k,v", "m,v", "k,m,v"):
        out = tmp_path / ("out_" + types.replace(",", ""))
        sh(KMX, "filter", "--in-matrix", run_dir, "--key", kfof, "--output", out, "--hard-min", "1", "--filter-batch-mb", "1", "--out-types", types)
        assert check_run(run_dir, out, False, key, 31, 1, types.replace(",", "")) > 0
    out = tmp_path / "out_g2"
    sh(KMX, "filter", "--in-matrix", run_dir, "--key", kfof, "--output", out, "--hard-min", "1", "--filter-batch-mb", "2", "--out-types", "k,m,v", "--gpus", "2")
    assert check_run(run_dir, out, False, key, 31, 1, "kmv") > 0


def test_driver_k96(inputs, tmp_path):
    rng = np.random.default_rng(8)
    genome = "".join(rng.choice(list("ACGT"), size=20000))
    def sample(seed, n):
        r = np.random.default_rng(seed)
        return [genome[a:a + 250] for a in r.integers(0, len(genome) - 250, n)]
    fof = tmp_path / "w.fof"; lines = []
    for i in range(3):
        fa = tmp_path / f"w{i}.fasta"; fa.write_text("".join(f">r{j}\n{s}\n" for j, s in enumerate(sample(i, 120)))); lines.append(f"W{i} : {fa}\n")
    fof.write_text("".join(lines))
    key = sample(77, 150)
    kf = tmp_path / "k.fasta"; kf.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(key)))
    kfof = tmp_path / "k.fof"; kfof.write_text(f"Q1 : {kf}\n")
    for mode in ("kmer:count:bin", "kmer:pa:bin"):
        run_dir = pipeline(inputs, tmp_path / f"run{mode[5]}", mode, 96, fof)
        out = tmp_path / f"out{mode[5]}"
        sh(KMX, "filter", "--in-matrix", run_dir, "--key", kfof, "--output", out, "--hard-min", "1", "--out-types", "k,m,v")
        assert check_run(run_dir, out, "pa" in mode, key, 96, 1, "kmv") > 0


def test_driver_one_byte_counts(inputs, tmp_path):
    """a count matrix with 1-byte counts written by hand (the header cannot say so: count_slots is the literal 1): --count-bytes 1"""
    run_dir = pipeline(inputs, tmp_path / "run", "kmer:count:bin")
    narrow = tmp_path / "narrow"
    shutil.copytree(run_dir, narrow)
    lists = key_counts(inputs[1], 31, 2)
    for p in range(P):
        hdr, body = read_matrix(run_dir / "matrices" / f"matrix_{p}.count", False)
        a = np.frombuffer(body, np.uint8).reshape(-1, 16)
        cols = np.minimum(np.ascontiguousarray(a[:, 8:]).view(np.uint32), 255).astype(np.uint8)
        (narrow / "matrices" / f"matrix_{p}.count").write_bytes(hdr + np.concatenate([a[:, :8], cols], axis=1).tobytes())
    out = tmp_path / "out"
    sh(KMX, "filter", "--in-matrix", narrow, "--key", inputs[0] / "key.fof", "--output", out, "--count-bytes", "1")
    for p in range(P):
        hdr, body = read_matrix(narrow / "matrices" / f"matrix_{p}.count", False)
        a = np.frombuffer(body, np.uint8).reshape(-1, 10)
        wide = a[:, 8:].astype(np.uint32).view(np.uint8).reshape(len(a), 8)
        em, ev, _, _ = fr.filter_expected(np.ascontiguousarray(a[:, :8]).view(np.uint64).reshape(-1, 1), wide, lists[p][0], lists[p][1], fr.MODE_COUNT)
        e = np.frombuffer(em, np.uint8).reshape(-1, 20)
        exp = np.concatenate([e[:, :8], np.minimum(np.ascontiguousarray(e[:, 8:]).view(np.uint32), 255).astype(np.uint8)], axis=1).tobytes()
        oh, ob = read_matrix(out / "matrices" / f"matrix_{p}.count", False)
        assert struct.unpack_from("<I", oh, 33)[0] == 3 and ob == exp
        assert open(out / "matrices" / f"{p}.vec").read() == "".join(f"{int(x)}\n" for x in ev)


def test_a_matrix_filtered_with_one_of_its_own_samples(inputs, tmp_path):
    """no restatement needed: soft-min 1, recurrence-min 1, the key = sample D1 at hard-min 1 -> k is empty, on every kept row the new
    column equals D1's column, and v equals that column wherever it is not 0"""
    run_dir = pipeline(inputs, tmp_path / "run", "kmer:count:bin", 31, None, "--soft-min", "1", "--recurrence-min", "1")
    (tmp_path / "d1.fof").write_text(f"D1 : {GD}/1.fasta\n")
    out = tmp_path / "out"
    sh(KMX, "filter", "--in-matrix", run_dir, "--key", tmp_path / "d1.fof", "--output", out, "--hard-min", "1", "--out-types", "k,m,v")
    rows = 0
    for p in range(P):
        f = kmfiles.read_kmer_file(out / "counts" / f"partition_{p}" / "D1.kmer")
        assert len(f["counts"]) == 0
        _, body = read_matrix(run_dir / "matrices" / f"matrix_{p}.count", False)
        col = np.frombuffer(body, np.uint8).reshape(-1, 16)[:, 8:12].copy().view(np.uint32).reshape(-1)
        _, ob = read_matrix(out / "matrices" / f"matrix_{p}.count", False)
        o = np.frombuffer(ob, np.uint8).reshape(-1, 20)
        assert np.array_equal(o[:, 8:12].copy().view(np.uint32), o[:, 16:20].copy().view(np.uint32))
        assert len(o) == int((col != 0).sum())
        v = np.array(open(out / "matrices" / f"{p}.vec").read().split(), np.uint32)
        assert np.array_equal(v, col)
        rows += len(o)
    assert rows > 0
