"""kmx_unitigs_* and kmx_groupsum_* on the MI355X against tests/unitig_ref.py: the C ABI through kmtricks_amd.lib on every case of
unitig_ref.cases() -- every output compared bit for bit with road A, the identities of the header on every result --, host and device
resident inputs, hashes cut to 0 and 3 bits, the launch shapes the knobs of unitigs.hip force, n = 0, the data errors, the limits; the
group-by at every column count on either side of a wave, windows, two calls against one, counts that sum past 2^32; the driver on runs
made from the golden samples and on a hand-made run whose table takes several windows.  Every assertion is exact.  Run with -m gpu."""
import ctypes as C
import os, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr
import unitig_ref as ur

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = ur.MODE_COUNT, ur.MODE_PA
OK, INVAL, UNSUP = 0, -2, -5
KNOBS = ("KMX_UNITIG_CUS", "KMX_UNITIG_GRID", "KMX_UNITIG_HASH_BITS")


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, k, what):
    assert out.n_unitigs == exp.U, f"{what}: {out.n_unitigs} unitigs, expected {exp.U}"
    for name, got, want, dt in (("unitig", out.unitig, exp.unitig, np.uint32), ("pos", out.pos, exp.pos, np.uint32), ("ori", out.ori, exp.ori, np.uint8),
                                ("start", out.start, exp.start, np.uint32), ("len", out.len, exp.len, np.uint32), ("circ", out.circ, exp.circ, np.uint8),
                                ("seq_off", out.seq_off, exp.seq_off(k), np.uint64)):
        want = np.array(want, dt)
        assert got.dtype == dt and got.tobytes() == want.tobytes(), f"{what}: {name}, first difference at {np.flatnonzero(got != want)[:3].tolist()}"
    assert [s.decode() for s in out.seqs] == exp.seqs, f"{what}: sequences"


def identical(a, b):
    return (a.n_unitigs == b.n_unitigs and all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("unitig", "pos", "ori", "start", "len", "circ", "seq_off"))
            and a.seqs == b.seqs)


def check_identities(out, keys, k):
    """len sums to n; unitig[start[u]] == u; pos is a permutation within each unitig; start ascends; the sequence's k-mers are the nodes'
    oriented keys"""
    n = len(keys)
    assert int(out.len.sum()) == n
    assert out.unitig[out.start].tolist() == list(range(out.n_unitigs))
    assert (np.diff(out.start.astype(np.int64)) > 0).all()
    order = np.lexsort((out.pos, out.unitig))
    assert out.pos[order].tolist() == [p for L in out.len.tolist() for p in range(L)]
    at = 0
    for u in range(out.n_unitigs):
        s = out.seqs[u].decode()
        assert len(s) == int(out.len[u]) + k - 1
        for p in range(int(out.len[u])):
            v = int(order[at + p])
            assert ur.enc(s[p:p + k]) == (keys[v] if out.ori[v] == 0 else ur.rc_int(keys[v], k)), (u, p)
        at += int(out.len[u])


@pytest.mark.parametrize("name", [c[0] for c in ur.cases()])
def test_case(ctx, name, monkeypatch):
    """every case of the list bit for bit against road A, with the identities"""
    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)
    _, k, keys = next(c for c in ur.cases() if c[0] == name)
    out = ctx.unitigs(ur.keys_to_words(keys, k), k)
    same(out, ur.expected(name), k, name)
    check_identities(out, keys, k)
    assert out.algo_bytes > len(keys) * 8 * ur.key_words_of(k)


def test_k_below_the_limit_is_refused_and_the_examples_at_their_k(ctx):
    """the header's worked examples are at k = 5, below the call's limit of 8: the call refuses them (tests/test_unitigs_cpu.py pins them
    on both roads)"""
    from kmtricks_amd import lib
    e = ur.EX_LINEAR
    with pytest.raises(lib.KmxError, match="kmer_size must be 8"):
        ctx.unitigs(ur.keys_to_words(list(e["keys"]), 5), 5)


DEV = ["seq_k31_shuffled", "seq_k64_shuffled", "seq_k97_sorted", "mixed_k31", "cycle_65", "dense_k8"]


@pytest.mark.parametrize("name", DEV)
def test_device_resident_keys(ctx, name):
    """the keys through _dev: the same result as _host; unitig_dev is the device array the copy came from"""
    import torch
    from kmtricks_amd import lib
    _, k, keys = next(c for c in ur.cases() if c[0] == name)
    words = ur.keys_to_words(keys, k)
    host = ctx.unitigs(words, k)
    d = torch.from_numpy(words.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    r = ctx.unitigs_dev(d.data_ptr(), len(keys), k, keep=True)
    try:
        r.wait()
        d.zero_()      # the call has copied the keys: the caller's may go before the sequences are asked for
        torch.cuda.synchronize()
        out = r.output()
        same(out, ur.expected(name), k, name)
        assert identical(out, host)
        back = np.zeros(len(keys), np.uint32)
        assert lib._lib.kmx_copy_to_host(ctx._h, back.ctypes.data, r.unitig_dev(), 4 * len(keys)) == 0 and back.tobytes() == out.unitig.tobytes()
    finally:
        r.free()


@pytest.mark.parametrize("bits", [0, 3])
@pytest.mark.parametrize("k", [31, 64])
def test_hash_bits(ctx, bits, k, monkeypatch):
    """KMX_UNITIG_HASH_BITS keeps the low bits of every hash and SETS the others: every probe chain starts in the table's last slots and
    wraps; n = 300 keeps the chains short.  Equal to road A and byte for byte to the call with the knob unset"""
    import random
    rng = random.Random(900 + k)
    keys = ur.ordered(ur.kmers_of(ur.rand_seq(rng, 299 + k), k)[:300], rng, True)
    assert len(keys) == 300
    exp = ur.unitigs_links(keys, k)
    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)
    base = ctx.unitigs(ur.keys_to_words(keys, k), k)
    same(base, exp, k, "knob unset")
    monkeypatch.setenv("KMX_UNITIG_HASH_BITS", str(bits))
    out = ctx.unitigs(ur.keys_to_words(keys, k), k)
    monkeypatch.delenv("KMX_UNITIG_HASH_BITS")
    same(out, exp, k, f"hash bits {bits}")
    assert identical(out, base)


@pytest.mark.parametrize("name", ["path_4097", "dense_k8", "cycle_1025"])
def test_launch_shapes(ctx, name, monkeypatch):
    """KMX_UNITIG_GRID=1 and KMX_UNITIG_CUS=1 (read per call): more than one trip of every stride loop -- nodes, states, tiles"""
    import torch
    _, k, keys = next(c for c in ur.cases() if c[0] == name)
    n = len(keys)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)
    base = ctx.unitigs(ur.keys_to_words(keys, k), k)
    same(base, ur.expected(name), k, "knobs unset")
    for env in (dict(KMX_UNITIG_GRID="1"), dict(KMX_UNITIG_CUS="1"), dict(KMX_UNITIG_CUS="1", KMX_UNITIG_GRID="1")):
        grid = 1 if "KMX_UNITIG_GRID" in env else 16 * (1 if "KMX_UNITIG_CUS" in env else n_cu)
        if "KMX_UNITIG_GRID" in env or n > 16 * 256:
            assert -(-n // (256 * grid)) > 1 or -(-2 * n // (256 * grid)) > 1, (env, n)
        for kn, v in env.items():
            monkeypatch.setenv(kn, v)
        out = ctx.unitigs(ur.keys_to_words(keys, k), k)
        for kn in env:
            monkeypatch.delenv(kn)
        same(out, ur.expected(name), k, env)
        assert identical(out, base)


def test_no_keys(ctx):
    out = ctx.unitigs(np.zeros((0, 1), np.uint64), 31)
    assert out.n_unitigs == 0 and len(out.unitig) == 0 and out.seq_off.tolist() == [0] and out.seqs == []


def task(lib, keys_ptr, n, k, kw=None, flags=0):
    return lib.KmxUnitigsTask(keys_ptr, n, k, ur.key_words_of(k) if kw is None else kw, flags, 0)


@pytest.mark.parametrize("what,match", [("duplicate", "occurs twice"), ("non-canonical", "not canonical"), ("high bits", "bits set from")])
def test_data_errors(ctx, what, match):
    """a duplicate, a key above its reverse complement, bits from 2k upwards: KMX_E_INVAL from _wait and from every accessor, the message
    naming the cause; the context stays usable"""
    import random
    from kmtricks_amd import lib
    k = 31
    rng = random.Random(77)
    keys = ur.kmers_of(ur.rand_seq(rng, 600), k)
    if what == "duplicate":
        keys[400] = keys[17]
    elif what == "non-canonical":
        keys[123] = ur.rc_int(keys[123], k)
        assert keys[123] > ur.canon_int(keys[123], k)
    else:
        keys[5] |= 1 << 62
    words = ur.keys_to_words(keys, k)
    t = task(lib, words.ctypes.data, len(keys), k)
    res = C.c_void_p()
    assert lib._lib.kmx_unitigs_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
    try:
        assert lib._lib.kmx_unitigs_result_wait(res) == INVAL
        assert match in lib._lib.kmx_last_error(ctx._h).decode()
        assert lib._lib.kmx_unitigs_result_wait(res) == INVAL
        buf = np.zeros(len(keys) + 1, np.uint64)
        for f in lib.UNITIGS_COPIES:
            assert getattr(lib._lib, "kmx_unitigs_result_copy_" + f)(res, buf.ctypes.data, len(buf)) == INVAL, f
        assert lib._lib.kmx_unitigs_result_n_unitigs(res) == 0 and lib._lib.kmx_unitigs_result_seq_bytes(res) == 0
        assert not lib._lib.kmx_unitigs_result_unitig_dev(res) and lib._lib.kmx_unitigs_result_algo_bytes(res) == 0
    finally:
        lib._lib.kmx_unitigs_result_free(res)
    with pytest.raises(lib.KmxError, match=match):
        ctx.unitigs(words, k)
    same(ctx.unitigs(ur.keys_to_words(ur.cases()[0][2], ur.cases()[0][1]), ur.cases()[0][1]), ur.expected(ur.cases()[0][0]), ur.cases()[0][1], "after the error")


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    one = np.zeros(4, np.uint64)

    def call(code, n=1, k=31, kw=None, flags=0, keys=one):
        for fn in (lib._lib.kmx_unitigs_host, lib._lib.kmx_unitigs_dev):
            t = task(lib, None if keys is None else keys.ctypes.data, n, k, kw, flags)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, n, k, kw, flags)

    call(INVAL, k=7); call(INVAL, k=128); call(INVAL, k=0)
    call(INVAL, k=31, kw=2); call(INVAL, k=32, kw=2); call(INVAL, k=33, kw=1); call(INVAL, k=127, kw=3); call(INVAL, k=64, kw=0)
    call(INVAL, keys=None)
    call(INVAL, flags=1); call(INVAL, flags=0x80000000)
    call(UNSUP, n=2 ** 31 - 1); call(UNSUP, n=2 ** 40)
    # a destination that is too small is refused; the context stays usable
    name, k, keys = ur.cases()[2]
    r = ctx.unitigs(ur.keys_to_words(keys, k), k, keep=True)
    small = np.zeros(len(keys) + 1, np.uint64)
    assert lib._lib.kmx_unitigs_result_copy_unitig(r._h, small.ctypes.data, len(keys) - 1) == INVAL
    assert lib._lib.kmx_unitigs_result_copy_start(r._h, small.ctypes.data, r.n_unitigs() - 1) == INVAL
    assert lib._lib.kmx_unitigs_result_copy_seq_off(r._h, small.ctypes.data, r.n_unitigs()) == INVAL
    assert lib._lib.kmx_unitigs_result_copy_seqs(r._h, small.ctypes.data, r.seq_bytes() - 1) == INVAL
    same(r.output(), ur.expected(name), k, name)
    r.free()


def test_kernel_times_with_profiling(ctx):
    from kmtricks_amd import lib
    name, k, keys = next(c for c in ur.cases() if c[0] == "path_4097")
    lib._lib.kmx_set_profiling(ctx._h, 1)
    try:
        r = ctx.unitigs(ur.keys_to_words(keys, k), k, keep=True)
        parts = r.kernel_parts_ms()
        assert len(parts) == 4 and r.kernel_ms() > 0 and all(p >= 0 for p in parts) and sum(parts) <= r.kernel_ms() * 1.01 + 0.01
        r.free()
    finally:
        lib._lib.kmx_set_profiling(ctx._h, 0)
    r = ctx.unitigs(ur.keys_to_words(keys, k), k, keep=True)
    assert r.kernel_ms() < 0 and r.kernel_parts_ms() == (-1.0,) * 4
    r.free()


# ---- kmx_groupsum_* ----------------------------------------------------------------------------------------------------------------
def labels(rng, n_rows, kind, n_labels=37):
    if kind == "one":          # every chunk's rows share a group
        return np.full(n_rows, 5, np.uint32)
    if kind == "distinct":     # no two neighbouring rows do
        return (np.arange(n_rows) % n_labels).astype(np.uint32)
    if kind == "runs":
        return np.repeat(rng.integers(0, n_labels, n_rows // 7 + 1), 7)[:n_rows].astype(np.uint32)
    g = rng.integers(0, n_labels, n_rows).astype(np.uint32)      # "random": with rows outside every window
    g[rng.random(n_rows) < 0.1] = 0xFFFFFFFF
    return g


def gs_same(out, exp, what):
    size, present, sums = exp
    assert out.size.dtype == np.uint32 and out.size.tobytes() == size.tobytes(), f"{what}: size"
    assert out.present.dtype == np.uint32 and out.present.shape == present.shape and out.present.tobytes() == present.tobytes(), f"{what}: present"
    assert (out.sums is None) == (sums is None), what
    if sums is not None:
        assert out.sums.dtype == np.uint64 and out.sums.tobytes() == sums.tobytes(), f"{what}: sums"


GS = [(COUNT, N, rows, kind) for N in (1, 63, 64, 65) for rows, kind in ((700, "random"), (257, "runs"))] + \
     [(PA, N, rows, kind) for N in (1, 511, 512, 513) for rows, kind in ((700, "random"), (257, "runs"))] + \
     [(COUNT, 130, 2100, "one"), (COUNT, 40, 2100, "distinct"), (PA, 40, 2100, "one"), (PA, 130, 2100, "distinct"), (COUNT, 9, 4200, "runs")]


@pytest.mark.parametrize("mode,N,rows,kind", GS)
def test_groupsum(ctx, mode, N, rows, kind):
    """columns on either side of a wave (COUNT) and of 64 payload bytes (PA); PA padding bits set; rows labelled 0xFFFFFFFF; the whole id
    range, windows that cut it, a list in another order and min_abund 2; host bodies at odd addresses"""
    rng = np.random.default_rng(1000 * N + rows)
    kw = 1 + N % 4
    body, counts = ur.make_body(rng, rows, N, kw, mode)
    g = labels(rng, rows, kind)
    want = mode == COUNT
    buf = np.zeros(len(body) + 8, np.uint8)
    for shift, (g0, G) in enumerate(((0, 37), (0, 11), (11, 20), (30, 100), (5, 1))):
        view = buf[shift % 4:shift % 4 + len(body)]
        view[:] = np.frombuffer(body, np.uint8)
        exp = ur.groupsum_np(counts, g, None, 1, g0, G, mode, want)
        gs_same(ctx.groupsum(view, rows, N, kw, mode, g, g0, G, sums=want), exp, (N, kind, g0, G))
    cols = rng.permutation(N)[:max(1, N - 3)].astype(np.uint32)
    a = 2 if mode == COUNT else 1
    exp = ur.groupsum_np(counts, g, cols, a, 0, 37, mode, False)
    loops = ur.groupsum_loops(counts, g, cols, a, 0, 37, mode, False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(exp[:2], loops[:2]))
    out = ctx.groupsum(body, rows, N, kw, mode, g, 0, 37, cols=cols, min_abund=a)
    gs_same(out, exp, (N, kind, "cols"))
    assert out.algo_bytes == rows * (len(body) // rows + 4) + 37 * (4 + 4 * len(cols))


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_groupsum_two_calls_equal_one_and_device_inputs(ctx, mode):
    """two partitions added into one set of device tables equal one call over both; rows and labels device resident at every alignment;
    counts of 2^32 - 1 sum past 2^32"""
    import torch
    from kmtricks_amd import lib
    rng = np.random.default_rng(31 + mode)
    N, kw, G = 67, 2, 23
    want = mode == COUNT
    (b1, c1), (b2, c2) = ur.make_body(rng, 900, N, kw, mode, big=True), ur.make_body(rng, 500, N, kw, mode, big=True)
    g1, g2 = labels(rng, 900, "runs", G), labels(rng, 500, "random", G)
    exp = ur.groupsum_np(np.concatenate([c1, c2]), np.concatenate([g1, g2]), None, 1, 0, G, mode, want)
    if want:
        assert int(exp[2].max()) > 2 ** 32
    gs_same(ctx.groupsum(b1 + b2, 1400, N, kw, mode, np.concatenate([g1, g2]), 0, G, sums=want), exp, "one call")
    first = ctx.groupsum(b1, 900, N, kw, mode, g1, 0, G, sums=want, keep=True)
    try:
        for shift in (0, 1, 3):
            d = torch.zeros(len(b2) + 8, dtype=torch.uint8, device="cuda:0")
            d[shift:shift + len(b2)] = torch.from_numpy(np.frombuffer(b2, np.uint8).copy()).to("cuda:0")
            dg = torch.from_numpy(g2.view(np.int32).copy()).to("cuda:0")
            torch.cuda.synchronize()
            if shift == 0:      # added to the first call's tables
                r = ctx.groupsum_dev(d.data_ptr(), 500, N, kw, mode, dg.data_ptr(), 0, G, sums=want, present_dev=first.present_dev(),
                                     sums_dev=first.sums_dev() if want else None, size_dev=first.size_dev(), keep=True)
                r.wait()
                assert r.present_dev() == first.present_dev() and r.size_dev() == first.size_dev()
                gs_same(r.output(), exp, "two calls")
                r.free()
                gs_same(first.output(), exp, "the first call's tables")
            else:
                gs_same(ctx.groupsum_dev(d.data_ptr() + shift, 500, N, kw, mode, dg.data_ptr(), 0, G, sums=want),
                        ur.groupsum_np(c2, g2, None, 1, 0, G, mode, want), ("dev", shift))
    finally:
        first.free()


def test_groupsum_launch_shapes(ctx, monkeypatch):
    """KMX_GROUPSUM_CUS=1 and KMX_GROUPSUM_GRID=1: several trips of the chunk loop"""
    rng = np.random.default_rng(5)
    for mode, N, rows in ((COUNT, 130, 4200), (PA, 40, 4200)):
        body, counts = ur.make_body(rng, rows, N, 1, mode)
        g = labels(rng, rows, "runs")
        exp = ur.groupsum_np(counts, g, None, 1, 0, 37, mode, mode == COUNT)
        for env in (dict(KMX_GROUPSUM_CUS="1"), dict(KMX_GROUPSUM_GRID="1")):
            for kn, v in env.items():
                monkeypatch.setenv(kn, v)
            out = ctx.groupsum(body, rows, N, 1, mode, g, 0, 37, sums=mode == COUNT)
            for kn in env:
                monkeypatch.delenv(kn)
            gs_same(out, exp, (mode, env))


def test_groupsum_limits_are_refused(ctx):
    from kmtricks_amd import lib
    g = np.zeros(8, np.uint32)
    dummy = np.zeros(64, np.uint8)

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, a=1, flags=0, n_rows=0, g0=0, G=4, groups=g, sums=None, rows=None):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        M = (N if cc is None else len(cc)) if M is None else M
        for fn in (lib._lib.kmx_groupsum_host, lib._lib.kmx_groupsum_dev):
            t = lib.KmxGroupsumTask(kw, mode, N, M, rows, n_rows, None if cc is None else cc.ctypes.data, None if groups is None else groups.ctypes.data, a, flags,
                                    g0, G, None, sums, None)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, a, flags, n_rows, g0, G)

    call(INVAL, N=0, cols=None); call(INVAL, M=0)
    call(INVAL, N=2, cols=(0, 1, 0)); call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4)); call(INVAL, cols=None, M=8)
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, mode=7)
    call(INVAL, a=0); call(INVAL, a=2, mode=PA)
    call(INVAL, flags=2); call(INVAL, flags=0x80000000)
    call(INVAL, G=0)
    call(INVAL, g0=2 ** 32 - 3, G=4)
    call(INVAL, mode=PA, flags=1)                                   # sums need counts
    call(INVAL, mode=PA, sums=0x1000); call(INVAL, sums=0x1000)     # a sums table with PA; a sums table without the flag
    call(INVAL, n_rows=5)                                           # rows without a pointer
    call(INVAL, n_rows=1, rows=dummy.ctypes.data, groups=None)      # labels without a pointer
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode)
    call(UNSUP, N=2 ** 30, cols=None)
    call(UNSUP, n_rows=2 ** 32)
    call(UNSUP, N=2 ** 20, cols=None, G=2 ** 13)                    # 2^33 table entries
    out = ctx.groupsum(b"", 0, 9, 1, COUNT, np.zeros(0, np.uint32), 3, 4, sums=True)      # n_rows = 0 is a valid call
    assert not out.size.any() and not out.present.any() and not out.sums.any() and out.present.shape == (4, 9)


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------------
IDS = ["D1", "D2"]


def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples, 4 partitions, with the fixture's repartition table: a count run, a
    presence/absence run, and the same presence/absence run made with --cpr"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxunitigs")
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
    return dict(dir=d, runs=runs, groups=d / "groups.txt")


@pytest.mark.parametrize("which", ["count", "pa_cpr"])
def test_driver_on_the_golden_samples(golden_runs, which, tmp_path):
    """FASTA and table against the restatement applied to the run's matrices: every k-mer, then the k-mers a `kmx diff` output of the same
    run lists (with two that the run lacks); every --value; --samples; --gpus 2"""
    run = golden_runs["runs"][which]
    mode = "kmer:count:bin" if which == "count" else "kmer:pa:bin"
    bodies, n, kw, rmode = dr.read_run_bodies(golden_runs["runs"]["count" if which == "count" else "pa"], mode, 4, 31)
    assert n == 2 and kw == 1
    fasta, table, _ = ur.driver_expected(bodies, n, kw, rmode, 31, ids=IDS)
    r = kmx("unitigs", "--run", run, "--output", tmp_path / "u.fa", "--table", tmp_path / "t.tsv", "-v")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert open(tmp_path / "u.fa").read() == fasta and fasta.count(">") >= 3
    assert open(tmp_path / "t.tsv").read() == table
    assert f"{fasta.count('>')} unitigs" in r.stderr
    values = ("mean", "frac", "sum", "present") if which == "count" else ("frac", "present")
    for value in values:
        exp = ur.driver_expected(bodies, n, kw, rmode, 31, value=value, ids=IDS)[1]
        r = kmx("unitigs", "--run", run, "--table", tmp_path / f"{value}.tsv", "--value", value, "--gpus", 2)
        assert r.returncode == 0 and open(tmp_path / f"{value}.tsv").read() == exp, (value, r.stderr)
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D2\n")
    a = 2 if which == "count" else 1
    exp = ur.driver_expected(bodies, n, kw, rmode, 31, cols=[1], min_abund=a, value="present", ids=IDS)[1]
    r = kmx("unitigs", "--run", run, "--table", tmp_path / "s.tsv", "--value", "present", "--samples", tmp_path / "s.txt", "--min-abund", a)
    assert r.returncode == 0 and open(tmp_path / "s.tsv").read() == exp, r.stderr
    # the k-mers of a kmx diff output of the same run, and two the run does not hold (one of them as its reverse complement, lower case)
    d = kmx("diff", "--run", run, "--groups", golden_runs["groups"], "--correction", "none", "--alpha", 0.9, "--output", tmp_path / "diff.tsv")
    assert d.returncode == 0, d.stderr
    text = open(tmp_path / "diff.tsv").read()
    listed = [ln.split("\t")[0] for ln in text.splitlines()[1:]]
    assert len(listed) > 20 and text.startswith("kmer\t")
    text += "A" * 31 + "\tnone\n" + ur.rc_str(listed[3]).lower() + "\n" + "ACGT" * 7 + "ACG\n"
    with open(tmp_path / "k.tsv", "w") as f:
        f.write(text)
    kmers = ur.parse_kmers(text, 31)
    fasta, table, missing = ur.driver_expected(bodies, n, kw, rmode, 31, kmers=kmers, ids=IDS)
    assert missing == 2
    r = kmx("unitigs", "--run", run, "--kmers", tmp_path / "k.tsv", "--output", tmp_path / "ku.fa", "--table", tmp_path / "kt.tsv", "--gpus", 2)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "ku.fa").read() == fasta and open(tmp_path / "kt.tsv").read() == table
    assert f"2 of the {len(kmers)} listed k-mers are not in the run" in r.stderr


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_driver_table_in_windows(tmp_path, mode):
    """a hand-made run of about 2500 unitigs in 3 partitions, 100 count columns or 300 presence/absence columns: --batch-mb 1 cuts the
    table into windows of 870 unitigs (1204 bytes of device tables each), every window re-reading the partitions; the same bytes as one
    window, on one shard and on two"""
    import random
    rng = random.Random(8 + mode)
    k, N = 31, 100 if mode == COUNT else 300
    parts = []
    for p in range(3):
        keys = set(ur.kmers_of(ur.rand_seq(rng, 400), k))
        while len(keys) < 1200:
            keys.add(ur.canon_int(rng.getrandbits(62), k))
        parts.append(sorted(keys))
    ids = [f"S{j}" for j in range(N)]
    nrng = np.random.default_rng(mode)
    bodies = []
    for p, keys in enumerate(parts):
        body, _ = ur.make_body(nrng, len(keys), N, 1, mode)
        a = np.frombuffer(body, np.uint8).reshape(len(keys), -1).copy()
        a[:, :8] = ur.keys_to_words(keys, k).view(np.uint8).reshape(len(keys), 8)
        bodies.append(a.reshape(-1))
    name = "kmer:count:bin" if mode == COUNT else "kmer:pa:bin"
    root = dr.write_run(tmp_path / "wide", name, k, ids, bodies)
    fasta, table, _ = ur.driver_expected(bodies, N, 1, mode, k, ids=ids)
    U = fasta.count(">")
    per_group = 4 + 4 * N + (8 * N if mode == COUNT else 0)
    assert U > (1 << 20) // per_group, "more unitigs than a window of 1 MB holds"
    one = kmx("unitigs", "--run", root, "--output", tmp_path / "u.fa", "--table", tmp_path / "one.tsv")
    assert one.returncode == 0, one.stderr
    assert open(tmp_path / "u.fa").read() == fasta and open(tmp_path / "one.tsv").read() == table
    for gpus in (1, 2):
        r = kmx("unitigs", "--run", root, "--table", tmp_path / f"w{gpus}.tsv", "--batch-mb", 1, "--gpus", gpus, "-v")
        assert r.returncode == 0, r.stderr
        assert f"windows of {(1 << 20) // per_group} unitigs" in r.stderr
        assert open(tmp_path / f"w{gpus}.tsv").read() == table
