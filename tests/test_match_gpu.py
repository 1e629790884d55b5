"""kmx_kset_* and kmx_match_* on the MI355X against tests/match_ref.py: the C ABI through kmtricks_amd.lib on every case of
match_ref.cases() -- every field of every record, every id, every occurrence count and the keys' ids compared bit for bit with road A --,
host and device resident inputs, hashes cut to 0 and 3 bits, the launch shapes the knobs of match.hip force, repeated builds of a set with
duplicates, occurrence tables that accumulate and carry past 2^32, the data errors, the limits; the driver on the golden samples and on
seeded reads in FASTA, FASTQ and gz.  Every assertion is exact.  Run with -m gpu."""
import ctypes as C
import gzip, os, random, subprocess
import numpy as np
import pytest

import match_ref as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
OK, INVAL, UNSUP = 0, -2, -5
KNOBS = ("KMX_MATCH_CUS", "KMX_MATCH_GRID", "KMX_MATCH_HASH_BITS")


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)


def recs_of(exp):
    from kmtricks_amd import lib
    return np.array(exp.recs, np.uint32).reshape(len(exp.recs), 6).view(lib.MATCH_REC).reshape(len(exp.recs))


def same(out, exp, what, ids=True, occ=True):
    want = recs_of(exp)
    assert out.recs.dtype == want.dtype and len(out.recs) == len(want), what
    bad = np.flatnonzero(out.recs != want)[:3]
    assert out.recs.tobytes() == want.tobytes(), f"{what}: recs differ first at reads {bad.tolist()}: {out.recs[bad].tolist()} for {want[bad].tolist()}"
    assert (out.total_kmers, out.total_hits) == (exp.total_kmers, exp.total_hits), what
    if ids:
        w = np.array(exp.ids, np.uint32)
        assert out.ids.dtype == np.uint32 and out.ids.tobytes() == w.tobytes(), f"{what}: ids, first difference at {np.flatnonzero(out.ids != w)[:3].tolist()}"
    else:
        assert out.ids is None
    if occ:
        w = np.array(exp.occ, np.uint64)
        assert out.occ.dtype == np.uint64 and out.occ.tobytes() == w.tobytes(), f"{what}: occ, first difference at {np.flatnonzero(out.occ != w)[:3].tolist()}"
    else:
        assert out.occ is None


def run_case(ctx, name, ids=True, occ=True):
    _, k, keys, reads = mr.case(name)
    s = ctx.kset(mr.keys_to_words(keys, k), k)
    try:
        exp = mr.expected(name)
        assert (s.n, s.n_distinct, s.kmer_size) == (len(keys), exp.n_distinct, k), name
        assert s.ids().tolist() == exp.key_ids, f"{name}: the keys' ids"
        out = ctx.match(s, reads, ids=ids, occ=occ)
        same(out, exp, name, ids, occ)
        return out
    finally:
        s.free()


@pytest.mark.parametrize("name", [c[0] for c in mr.cases()])
def test_case(ctx, name):
    """every case of the list bit for bit against road A, ids and occurrences asked for"""
    out = run_case(ctx, name)
    _, k, keys, reads = mr.case(name)
    nb = sum(len(r) for r in reads)
    assert out.algo_bytes >= nb + 8 * out.total_kmers + 8 * mr.key_words_of(k) * out.total_hits + 24 * len(reads) + 4 * nb + 8 * out.total_hits


@pytest.mark.parametrize("name", ["tiles_k31", "words_k97", "cover_k127_all", "dups_k31", "many_reads_k12"])
@pytest.mark.parametrize("ids,occ", [(False, False), (True, False), (False, True)])
def test_ids_and_occ_on_and_off(ctx, name, ids, occ):
    """the records do not depend on what else is asked for"""
    run_case(ctx, name, ids=ids, occ=occ)


def test_k_below_the_limit_is_refused(ctx):
    """the header's worked example is at k = 5, below the call's limit of 8: the call refuses it (tests/test_match_cpu.py pins it on both
    roads)"""
    from kmtricks_amd import lib
    with pytest.raises(lib.KmxError, match="kmer_size must be 8"):
        ctx.kset(mr.keys_to_words(list(mr.EXAMPLE["keys"]), 5), 5)


def test_repeated_builds_give_the_least_indices(ctx):
    """1 to 50 copies of a key spread over the list: whatever thread wins a slot, the id is the least index"""
    _, k, keys, _ = mr.case("dups_k31")
    want = mr.expected("dups_k31").key_ids
    words = mr.keys_to_words(keys, k)
    for _ in range(3):
        s = ctx.kset(words, k)
        try:
            assert s.ids().tolist() == want and s.n_distinct == 60
        finally:
            s.free()


@pytest.mark.parametrize("bits", [0, 3])
@pytest.mark.parametrize("name", ["n300_k31", "n300_k64", "dups_k31"])
def test_hash_bits(ctx, bits, name, monkeypatch):
    """KMX_MATCH_HASH_BITS keeps the low bits of every hash and SETS the others, for slot and tag: every probe chain starts in the table's
    last slots and wraps, every tag (0 bits) or every eighth (3) is equal, so every look-up confirms keys that are not its own"""
    monkeypatch.setenv("KMX_MATCH_HASH_BITS", str(bits))
    run_case(ctx, name)


@pytest.mark.parametrize("knob,value", [("KMX_MATCH_CUS", "1"), ("KMX_MATCH_GRID", "1")])
@pytest.mark.parametrize("name", ["long_read_k31", "many_reads_k12", "set_n4097", "tiles_k8"])
def test_launch_knobs(ctx, knob, value, name, monkeypatch):
    """one CU's worth of workgroups, and one workgroup: the kernels stride over their work"""
    monkeypatch.setenv(knob, value)
    run_case(ctx, name)


@pytest.mark.parametrize("name", ["tiles_k31", "words_k65", "cover_k127_gap0", "dups_k31", "set_n0", "no_reads"])
def test_device_resident_inputs(ctx, name):
    """keys and reads through _dev: the same as _host; the caller's keys are zeroed once the build has been waited for"""
    import torch
    _, k, keys, reads = mr.case(name)
    exp = mr.expected(name)
    words = mr.keys_to_words(keys, k)
    dk = torch.from_numpy(words.view(np.int64).copy().reshape(-1)).to("cuda:0") if len(keys) else None
    torch.cuda.synchronize()
    s = ctx.kset_dev(dk.data_ptr() if dk is not None else None, len(keys), k)
    try:
        s.wait()
        if dk is not None:
            dk.zero_()
            torch.cuda.synchronize()
        assert s.ids().tolist() == exp.key_ids and s.n_distinct == exp.n_distinct
        blob, offs = ctx.pack_reads(reads)
        db = torch.from_numpy(np.frombuffer(blob if blob else b"N", np.uint8).copy()).to("cuda:0")
        do = torch.from_numpy(offs.view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        out = ctx.match_dev(s, db.data_ptr(), do.data_ptr(), len(reads), ids=True, occ=True)
        same(out, exp, name)
    finally:
        s.free()


def test_occ_accumulates_and_carries(ctx):
    """two calls into one table equal one call over all the reads; a table seeded with 2^32 - 1 carries into the high word"""
    import torch
    from kmtricks_amd import lib
    _, k, keys, reads = mr.case("tiles_k31")
    exp = mr.expected("tiles_k31")
    half = len(reads) // 2
    s = ctx.kset(mr.keys_to_words(keys, k), k)
    try:
        seed = (1 << 32) - 1
        table = torch.full((len(keys),), seed, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for part in (reads[:half], reads[half:]):
            r = ctx.match(s, part, occ_dev=table.data_ptr(), keep=True)
            try:
                assert r.occ_dev() == table.data_ptr()
            finally:
                r.free()
        torch.cuda.synchronize()
        got = table.cpu().numpy().view(np.uint64)
        assert got.tolist() == [seed + x for x in exp.occ]
        assert any(x >> 32 for x in got.tolist())
        a, b = mr.match_strings(keys, k, reads[:half]), mr.match_strings(keys, k, reads[half:])
        assert [x + y for x, y in zip(a.occ, b.occ)] == exp.occ
        with pytest.raises(lib.KmxError, match="an occ table without KMX_MATCH_OCC"):
            t = lib.KmxMatchTask(s._h, None, np.zeros(1, np.uint64).ctypes.data, 0, 0, 0, table.data_ptr(), 0)
            res = C.c_void_p()
            ctx._check(lib._lib.kmx_match_host(ctx._h, C.byref(t), C.byref(res)), "kmx_match_host")
    finally:
        s.free()


def test_contention_on_one_key(ctx):
    """one key hit 10^5 times by a poly-A read, and 470 times on the other strand"""
    out = run_case(ctx, "poly_a_k31")
    assert int(out.occ[0]) == mr.POLY_HITS + 470 and int(out.recs["hits"][0]) == mr.POLY_HITS == int(out.recs["fwd"][0]) and int(out.recs["fwd"][2]) == 0


def kset_rc(ctx, words, n, k, kw=None, flags=0):
    from kmtricks_amd import lib
    t = lib.KmxKsetTask(words.ctypes.data if words is not None else None, n, k, lib.key_words_of(k) if kw is None else kw, flags, 0)
    h = C.c_void_p()
    rc = lib._lib.kmx_kset_host(ctx._h, C.byref(t), C.byref(h))
    return rc, h, lib._lib.kmx_last_error(ctx._h).decode()


def test_data_errors(ctx):
    """a key with bits from 2 k upwards; a key greater than its reverse complement: found on the device, returned by the wait, by every
    accessor and by a match call on the set"""
    from kmtricks_amd import lib
    good = mr.distinct(mr.kmers_of([mr.rand_seq(random.Random(5), 200)], 31))
    nc = next(x for x in (mr.enc(mr.rc_str(mr.dec(g, 31))) for g in good) if x != mr.canon_of(mr.dec(x, 31)))
    for bad, text in ((good[3] | 1 << 62, "kmx_kset: a key has bits set from 2 * kmer_size upwards"),
                      (nc, "kmx_kset: a key is not canonical (it is greater than its reverse complement)")):
        keys = good[:100] + [bad] + good[100:]
        rc, h, _ = kset_rc(ctx, mr.keys_to_words(keys, 31), len(keys), 31)
        assert rc == OK
        try:
            assert lib._lib.kmx_kset_wait(h) == INVAL and lib._lib.kmx_last_error(ctx._h).decode() == text
            assert lib._lib.kmx_kset_wait(h) == INVAL and lib._lib.kmx_kset_n_distinct(h) == 0 and lib._lib.kmx_kset_n(h) == 0
            ids = np.zeros(len(keys), np.uint32)
            assert lib._lib.kmx_kset_copy_ids(h, ids.ctypes.data, ids.size) == INVAL
            blob, offs = ctx.pack_reads(["ACGT" * 20])
            bases = np.frombuffer(blob, np.uint8)
            t = lib.KmxMatchTask(h, bases.ctypes.data, offs.ctypes.data, 1, 0, 0, None, 0)
            res = C.c_void_p()
            assert lib._lib.kmx_match_host(ctx._h, C.byref(t), C.byref(res)) == INVAL and lib._lib.kmx_last_error(ctx._h).decode() == text
            assert not res.value
        finally:
            lib._lib.kmx_kset_free(h)


def test_limits(ctx):
    """every limit with its code, each refused before any GPU work"""
    from kmtricks_amd import lib
    w = mr.keys_to_words([5], 31)
    for args, code, text in (((w, 1, 7), INVAL, "kmx_kset_host: kmer_size must be 8 ... 127"), ((w, 1, 128), INVAL, "kmx_kset_host: kmer_size must be 8 ... 127"),
                             ((w, 1, 31, 2), INVAL, "kmx_kset_host: key_words must be ceil(kmer_size / 32)"), ((None, 1, 31), INVAL, "kmx_kset_host: null keys"),
                             ((w, 1, 31, None, 4), INVAL, "kmx_kset_host: unknown flag bits"),
                             ((w, (1 << 31) + 1, 31), UNSUP, "kmx_kset_host: more than 2^31 k-mers in one set")):
        rc, h, err = kset_rc(ctx, *args)
        assert rc == code and not h.value and err.startswith(text), (args[1:], rc, err)
    s = ctx.kset(w, 31)
    other = lib.Context(0)
    try:
        offs = np.array([0, 1], np.uint64)
        base = np.frombuffer(b"A", np.uint8)
        A = base.ctypes.data
        res = C.c_void_p()

        def call(c, set_h, bases, offsets, n_seqs, flags, occ=None):
            t = lib.KmxMatchTask(set_h, bases, offsets, n_seqs, flags, 0, occ, 0)
            rc = lib._lib.kmx_match_host(c._h, C.byref(t), C.byref(res))
            assert not res.value
            return rc, lib._lib.kmx_last_error(c._h).decode()
        assert call(ctx, None, A, offs.ctypes.data, 1, 0) == (INVAL, "kmx_match_host: null set")
        assert call(other, s._h, A, offs.ctypes.data, 1, 0) == (INVAL, "kmx_match_host: the set belongs to another context")
        assert call(ctx, s._h, A, offs.ctypes.data, 1, 4) == (INVAL, "kmx_match_host: unknown flag bits")
        assert call(ctx, s._h, None, offs.ctypes.data, 1, 0) == (INVAL, "kmx_match_host: null reads")
        assert call(ctx, s._h, A, None, 0, 0) == (INVAL, "kmx_match_host: null reads")
        assert call(ctx, s._h, A, offs.ctypes.data, 1, 0, offs.ctypes.data) == (INVAL, "kmx_match_host: an occ table without KMX_MATCH_OCC")
        assert call(ctx, s._h, A, offs.ctypes.data, 1 << 31, 0) == (UNSUP, "kmx_match_host: 2^31 queries and more in one call (send them in batches)")
        big = np.array([0, 1 << 32], np.uint64)
        assert call(ctx, s._h, A, big.ctypes.data, 1, 0) == (UNSUP, "kmx_match_host: 2^32 bases and more in one call (send the queries in batches)")
        one = np.array([1, 2], np.uint64)
        assert call(ctx, s._h, A, one.ctypes.data, 1, 0) == (INVAL, "kmx_match_host: offsets[0] must be 0")
        out = ctx.match(s, ["ACGT"])      # without ids and occ: the accessors refuse, the records are there
        assert out.ids is None and out.occ is None and out.recs.tolist() == [(0, 0, 0, 0, mr.NONE, mr.NONE)]
        r = ctx.match(s, ["ACGT"], keep=True)
        try:
            a = np.zeros(4, np.uint32)
            assert lib._lib.kmx_match_result_copy_ids(r._h, a.ctypes.data, 4) == INVAL and "without KMX_MATCH_IDS" in lib._lib.kmx_last_error(ctx._h).decode()
            assert lib._lib.kmx_match_result_copy_occ(r._h, a.ctypes.data, 4) == INVAL and "without KMX_MATCH_OCC" in lib._lib.kmx_last_error(ctx._h).decode()
            assert not r.occ_dev()
        finally:
            r.free()
    finally:
        s.free()
        other.close()


def test_profiling_parts(ctx):
    """with profiling on the two parts are there and sum to no more than the whole"""
    ctx.set_profiling(True)
    try:
        _, k, keys, reads = mr.case("many_reads_k12")
        s = ctx.kset(mr.keys_to_words(keys, k), k)
        try:
            assert s.kernel_ms >= 0
            r = ctx.match(s, reads, keep=True)
            try:
                probe, cover = r.kernel_parts_ms()
                assert probe >= 0 and cover >= 0 and probe + cover <= r.kernel_ms() * 1.01 + 0.01
            finally:
                r.free()
        finally:
            s.free()
    finally:
        ctx.set_profiling(False)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def read_text(path):
    raw = open(path, "rb").read()
    return (gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw).decode()


def check_driver(tmp_path, tag, set_args, keys, k, read_files, extra=(), rule=None, road=mr.match_strings):
    """`kmx match` with all four outputs, each byte for byte against tests/match_ref.py -> (the restatement's result, stderr)"""
    recs = [r for f in read_files for r in mr.parse_records(read_text(f))]
    heads, reads, quals = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
    exp = road(keys, k, reads)
    o = {n: tmp_path / f"{tag}.{n}" for n in ("out", "ext", "cnt", "pos")}
    r = kmx("match", *set_args, *[a for f in read_files for a in ("--reads", f)], "--output", o["out"], "--extract", o["ext"], "--kmer-counts", o["cnt"],
            "--positions", o["pos"], *extra)
    assert r.returncode == 0 and r.stdout == "", (tag, r.stderr)
    assert open(o["out"]).read() == mr.output_text(heads, reads, exp.recs), tag
    assert open(o["ext"]).read() == mr.extract_text(heads, reads, quals, exp.recs, **(rule or {})), tag
    assert open(o["cnt"]).read() == mr.kmer_counts_text(keys, k, exp.key_ids, exp.occ), tag
    assert open(o["pos"]).read() == mr.positions_text(k, reads, exp.ids), tag
    return exp, r.stderr


def write_fasta(path, recs, width=None, crlf=False):
    nl = "\r\n" if crlf else "\n"
    with open(path, "w", newline="") as f:
        for h, s in recs:
            lines = [s] if not width else [s[i:i + width] for i in range(0, len(s), width)] or [""]
            f.write(h + nl + "".join(x + nl for x in lines))


def write_fastq(path, recs, rng):
    with open(path, "w") as f:
        for h, s in recs:
            f.write(f"@{h[1:]}\n{s}\n+\n{''.join(rng.choice('#5?@IJ') for _ in s)}\n")


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples, 4 partitions, with the fixture's repartition table: a count run, a
    presence/absence run and the same made with --cpr; a `kmx diff` output and a `kmx unitigs --output` of the count run; seeded reads"""
    import struct
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxmatch")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    with open(d / "groups.txt", "w") as f:
        f.write("D1 control\nD2\tcase\n")
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    runs = {}
    for name, mode, extra in (("count", "kmer:count:bin", []), ("pa", "kmer:pa:bin", []), ("pa_cpr", "kmer:pa:bin", ["--cpr"])):
        r = kmx(*base, "--run-dir", d / name, "--mode", mode, *extra)
        assert r.returncode == 0, r.stderr
        runs[name] = d / name
    r = kmx("diff", "--run", runs["count"], "--groups", d / "groups.txt", "--correction", "none", "--alpha", 0.9, "--output", d / "diff.tsv")
    assert r.returncode == 0, r.stderr
    r = kmx("unitigs", "--run", runs["count"], "--output", d / "unitigs.fa")
    assert r.returncode == 0, r.stderr
    # seeded reads: pieces of the golden samples on either strand, in either case, with an N, between random reads
    rng = random.Random(77)
    src = [s for f in ("1.fasta", "2.fasta") for _, s, _ in mr.parse_records(read_text(os.path.join(GD, f)))]
    recs = []
    for i in range(60):
        kind = i % 4
        s = mr.rand_seq(rng, rng.randrange(20, 160))
        if kind:
            piece = rng.choice(src)
            a = rng.randrange(0, len(piece) - 40)
            piece = piece[a:a + rng.randrange(31, 70)]
            piece = mr.rc_str(piece) if kind == 2 else piece.lower() if kind == 3 else piece
            s = s[:len(s) // 2] + piece + ("N" if i % 5 == 0 else "") + s[len(s) // 2:]
        recs.append((f">s{i} seeded read {i}" if i % 3 else f">s{i}", s))
    recs.append((">empty", ""))
    write_fasta(d / "seeded.fa", recs, width=60)
    return dict(dir=d, runs=runs, diff=d / "diff.tsv", unitigs=d / "unitigs.fa", seeded=d / "seeded.fa", recs=recs,
                reads=[os.path.join(GD, "1.fasta"), os.path.join(GD, "2.fasta"), d / "seeded.fa"])


def run_keys(run, mode):
    """the row keys of a run's partitions, partition ascending, file order"""
    import dist_ref as dr
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, 4, 31)
    rb = dr.row_bytes(kw, n, rmode)
    assert kw == 1
    return [int(x) for b in bodies for x in np.frombuffer(dr.as_bytes(b), np.uint8).reshape(-1, rb)[:, :8].copy().view(np.uint64).reshape(-1)]


def test_driver_set_from_a_kmer_list(golden, tmp_path):
    """--kmers: a `kmx diff` output of the golden run, with a k-mer a second time, one as its lower-case reverse complement, one no read holds"""
    text = open(golden["diff"]).read()
    listed = [ln.split("\t")[0] for ln in text.splitlines()[1:]]
    assert len(listed) > 20 and text.startswith("kmer\t")
    text += listed[2] + "\tagain\n" + mr.rc_str(listed[5]).lower() + "\n" + "ACGT" * 7 + "ACG\n"
    with open(tmp_path / "k.tsv", "w") as f:
        f.write(text)
    k, keys = mr.parse_kmers(text)
    assert k == 31 and len(keys) == len(listed) + 3
    exp, err = check_driver(tmp_path, "kmers", ["--kmers", tmp_path / "k.tsv"], keys, 31, golden["reads"], extra=["-v"])
    assert exp.n_distinct == len(listed) + 1 and exp.total_hits > 50 and exp.occ[-1] == 0 and exp.occ[-2] == 0 and exp.occ[-3] == 0
    assert f"a set of {len(keys)} k-mers ({exp.n_distinct} distinct), k = 31" in err and f"{exp.total_kmers} k-mers, {exp.total_hits} hits" in err


def test_driver_set_from_sequences(golden, tmp_path):
    """--seqs: every k-mer of every unitig of the golden run, duplicates and all"""
    seqs = [s for _, s, _ in mr.parse_records(read_text(golden["unitigs"]))]
    keys = mr.kmers_of(seqs, 31)
    assert len(seqs) >= 3 and len(keys) > 100
    exp, _ = check_driver(tmp_path, "seqs", ["--seqs", golden["unitigs"], "--kmer-size", 31], keys, 31, golden["reads"])
    assert exp.total_hits > 100
    keys12 = mr.kmers_of(seqs, 12)      # at another k the same file is another set, with repeats
    exp, _ = check_driver(tmp_path, "seqs12", ["--seqs", golden["unitigs"], "--kmer-size", 12], keys12, 12, golden["reads"])
    assert exp.n_distinct < len(keys12)


@pytest.mark.parametrize("which", ["count", "pa_cpr"])
def test_driver_set_from_a_run(golden, which, tmp_path):
    """--run: every row key of a count run and of a presence/absence run made with --cpr"""
    keys = run_keys(golden["runs"]["count" if which == "count" else "pa"], "kmer:count:bin" if which == "count" else "kmer:pa:bin")
    exp, _ = check_driver(tmp_path, which, ["--run", golden["runs"][which]], keys, 31, golden["reads"], extra=["--gpus", 2])
    assert exp.n_distinct == len(keys) > 100 and exp.total_hits > 100


@pytest.mark.parametrize("rule,args", [(dict(min_hits=3), ["--min-hits", 3]), (dict(min_frac=0.25), ["--min-frac", 0.25]), (dict(min_cover=0.3), ["--min-cover", 0.3]),
                                       (dict(invert=True), ["--invert"]), (dict(min_hits=0, min_frac=0.0, min_cover=0.0), ["--min-hits", 0, "--min-frac", 0, "--min-cover", 0]),
                                       (dict(min_hits=2, min_frac=0.1, min_cover=0.5, invert=True), ["--min-hits", 2, "--min-frac", 0.1, "--min-cover", 0.5, "--invert"])])
def test_driver_keep_rule(golden, rule, args, tmp_path):
    keys = run_keys(golden["runs"]["count"], "kmer:count:bin")
    exp, _ = check_driver(tmp_path, "rule", ["--run", golden["runs"]["count"]], keys, 31, golden["reads"], extra=args, rule=rule)
    recs = [r for f in golden["reads"] for r in mr.parse_records(read_text(f))]
    kept = [mr.kept(r, len(s[1]), **rule) for r, s in zip(exp.recs, recs)]
    assert any(kept) and not all(kept)


def test_driver_read_formats(golden, tmp_path):
    """the seeded reads as FASTA in one line and in lines of 60 with CRLF, as FASTQ, each plain and gz; several files, the read index running on"""
    rng = random.Random(5)
    recs = golden["recs"]
    write_fasta(tmp_path / "one.fa", recs)
    write_fasta(tmp_path / "crlf.fa", recs, width=60, crlf=True)
    write_fastq(tmp_path / "r.fq", recs, rng)
    for name in ("one.fa", "crlf.fa", "r.fq"):
        with open(tmp_path / name, "rb") as f, gzip.open(tmp_path / (name + ".gz"), "wb") as g:
            g.write(f.read())
    keys = run_keys(golden["runs"]["count"], "kmer:count:bin")
    files = [tmp_path / n for n in ("one.fa", "r.fq.gz", "crlf.fa.gz", "r.fq", "one.fa.gz", "crlf.fa")]
    exp, _ = check_driver(tmp_path, "formats", ["--run", golden["runs"]["count"]], keys, 31, files)
    n = len(recs)
    assert len(exp.recs) == 6 * n and all(exp.recs[q] == exp.recs[q % n] for q in range(6 * n))
    ext = open(tmp_path / "formats.ext").read()
    assert "\n+\n" in ext and ext.count("\n@s") + ext.count("\n>s") + 1 == sum(1 for r in exp.recs if r[1])


@pytest.mark.parametrize("gpus", [1, 2])
def test_driver_batches(tmp_path, gpus):
    """--batch-mb 1: three batches -- 300 reads, a read larger than a batch that goes alone, 300 reads --, on one device context and round-robin
    on two; the outputs stay in input order and the occurrence tables of the batches add up.  (Road B: 1.4 Mbp take road A too long.)"""
    rng = random.Random(9)
    big = mr.rand_seq(rng, 1100000)
    small = [mr.rand_seq(rng, 500) for _ in range(600)]
    recs = [(f">a{i}", s) for i, s in enumerate(small[:300])] + [(">big one", big)] + [(f">b{i} x", s) for i, s in enumerate(small[300:])]
    write_fasta(tmp_path / "reads.fa", recs)
    pieces = small[::40] + [big[i:i + 100] for i in range(0, len(big), 50000)]
    keys = mr.kmers_of(pieces, 31)
    keys += keys[:50]
    with open(tmp_path / "k.tsv", "w") as f:
        f.write("".join(mr.dec(x, 31) + "\n" for x in keys))
    exp, err = check_driver(tmp_path, f"b{gpus}", ["--kmers", tmp_path / "k.tsv"], keys, 31, [tmp_path / "reads.fa"], extra=["--batch-mb", 1, "--gpus", gpus, "-v"],
                            road=mr.match_numpy)
    assert "601 reads in 3 batches" in err and exp.total_hits >= len(keys) - 50
