"""Every count entry point over the whole window-hash range (tests/synth.py's window shapes: windows of 2^32 and beyond, window * P
on both sides of 2^63 and 2^64, partition ids up to 2^64 - 1, the all-ones key) and at extreme counts (65535 ... 65537 and above
2^24 on genome-length records), each bucket kernel forced in turn, keys and counts against the oracle."""
import numpy as np
import pytest

import orc
from synth import WINDOW_SHAPES, U64, hash_window, value_xxh64, canonical_value
from test_count_gpu import random_reads

pytestmark = pytest.mark.gpu

K, M, P = 31, 10, 4
MANY, FEW = 1500, 3                # copies of the chosen k-mer: its bucket beyond the wave kernels (> 1024 keys), or counted by them
FUSED_SHAPES = [s for s in WINDOW_SHAPES if s not in ("sparse-ids", "all-ones-top")]      # (the fused calls' window id is the partition)


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _chosen(reads, k):
    """the first k-mer of the reads whose XXH64 is below 2^63 (both all-ones constructions apply to it) -> (string, XXH64)"""
    for r in reads:
        for j in range(0, len(r) - k + 1, 7):
            s = r[j:j + k]
            if "N" not in s:
                x = value_xxh64(canonical_value(s), k)
                if x < 1 << 63:
                    return s, x
    raise AssertionError("no k-mer")


_DATA = {}


def dataset(copies):
    """reads of ~700 k k-mers (four partitions of hundreds of buckets each), the chosen k-mer added `copies` times, and a repartition
    table that sends the chosen k-mer to partition 1 -> (reads, table, chosen XXH64, oracle streams)"""
    if copies not in _DATA:
        reads = random_reads(5150, 2400, 150, n_rate=0.002) * 2
        s, x = _chosen(reads, K)
        lut, rep = orc.minimizer_lut(M), orc.repart_static(M, P)
        rep[orc.minimizer_of(orc.kmer_from_string(s), K, M, lut)] = 1
        reads = reads + [s] * copies
        exp = orc.superk_partition(reads, K, M, lut, rep, P)
        assert orc.superk_partition([s], K, M, lut, rep, P)[1][1] == 1      # (the chosen k-mer is partition 1's)
        _DATA[copies] = (reads, rep, x, exp)
    return _DATA[copies]


def _expect(exp, W, ids, hard_min):
    return [orc.count_hash(exp[p][0], K, W, ids[p], hard_min) for p in range(P)]


def _same(got, want, what):
    for p in range(P):
        gk, gc = got[p]
        ek, ec = want[p]
        assert np.array_equal(np.asarray(gk).reshape(-1), ek) and np.array_equal(gc, ec), (what, p, len(gc), len(ec))


def _check_all_ones(want, shape, copies):
    if shape.startswith("all-ones"):      # (the oracle's own answer: the chosen k-mer's key is the all-ones one, with its count)
        ek, ec = want[1]
        assert int(ek[-1]) == U64 and int(ec[-1]) >= copies


@pytest.mark.parametrize("path", ["waves", "lds-hash", "lds-sort", "library"])
@pytest.mark.parametrize("shape,copies", [(s, MANY) for s in WINDOW_SHAPES] + [("all-ones-top", FEW), ("all-ones-one", FEW)])
def test_count_batch_and_hash_over_the_key_space(ctx, monkeypatch, shape, copies, path):
    """kmx_count_batch (partition ids of the shape) and kmx_count_hash (one call per partition): the sample sort with the wave kernels and
    the LDS kernels behind them (default), every bucket by the LDS hash set or the LDS sort (KMX_COUNT_BUCKETS=hash|sort), and the library
    radix sort (KMX_COUNT_SORT=library: its key width comes from window * (largest id + 1))"""
    if path == "library":
        monkeypatch.setenv("KMX_COUNT_SORT", "library")
    if path.startswith("lds-"):
        monkeypatch.setenv("KMX_COUNT_BUCKETS", path[4:])
    reads, rep, x, exp = dataset(copies)
    W, ids = hash_window(shape, P, x, at=1)
    want = _expect(exp, W, ids, 1)
    _check_all_ones(want, shape, copies)
    _same(ctx.count_batch([e[0] for e in exp], K, 1, window=W, partitions=ids), want, "kmx_count_batch")
    want2 = _expect(exp, W, ids, 2)
    _same([ctx.count_hash(exp[p][0], K, W, ids[p], 2) for p in range(P)], want2, "kmx_count_hash")
    if shape in ("2^40", "above-2^64", "sparse-ids"):
        assert max(int(w[0].max()) for w in want) >= 1 << 36


ENTRIES = ["reads", "reads-streams", "dev-counting-first", "dev-full-sort", "dev-no-table", "dev-two-walks", "dev-multi"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape,copies", [(s, MANY) for s in FUSED_SHAPES] + [("all-ones-one", FEW)])
def test_fused_count_over_the_key_space(ctx, monkeypatch, capfd, shape, copies, entry):
    """kmx_count_reads (with and without streams), kmx_count_reads_dev on the sync-free path (counting first, KMX_COUNT_HASH_FIRST=1; the
    full sort, =0; without the bucket look-up table, KMX_COUNT_LUT=0) and on the two-walk path (KMX_COUNT_FAST=0), and
    kmx_count_reads_dev_multi: window id = partition, the all-ones key built with partition id 1.  KMX_TRACE names the path that ran."""
    from kmtricks_amd import lib
    reads, rep, x, exp = dataset(copies)
    W, ids = hash_window(shape, P, x, at=1)[0], list(range(P))
    want = _expect(exp, W, ids, 1)
    _check_all_ones(want, shape, copies)
    monkeypatch.setenv("KMX_TRACE", "1")
    if entry.startswith("reads"):
        got, nk, streams, _ = ctx.count_reads(reads, K, M, rep, P, 1, window=W, streams=entry == "reads-streams")
        assert nk == [e[1] for e in exp] and (streams is None or streams == [e[0] for e in exp])
        _same(got, want, entry)
        return
    monkeypatch.setenv("KMX_COUNT_HASH_FIRST", "0" if entry == "dev-full-sort" else "1")
    if entry == "dev-no-table":
        monkeypatch.setenv("KMX_COUNT_LUT", "0")
    if entry == "dev-two-walks":
        monkeypatch.setenv("KMX_COUNT_FAST", "0")
    store = lib.Store(0)
    try:
        capfd.readouterr()
        if entry == "dev-multi":
            half = reads[::2]
            exp2 = orc.superk_partition(half, K, M, orc.minimizer_lut(M), rep, P)
            res = ctx.count_reads_dev_multi([reads, half], K, M, rep, P, 1, [store], window=W)
            for (lists, nk, _, _), e, w in ((res[0], exp, want), (res[1], exp2, _expect(exp2, W, ids, 1))):
                assert nk == [x_[1] for x_ in e]
                _same([ctx.read_list(lists[p][0], lists[p][1], 1) for p in range(P)], w, entry)
            return
        lists, nk, _ = ctx.count_reads_dev(reads, K, M, rep, P, 1, [store], window=W)
        assert nk == [e[1] for e in exp]
        _same([ctx.read_list(lists[p][0], lists[p][1], 1) for p in range(P)], want, entry)
        err = capfd.readouterr().err
        if entry == "dev-two-walks":
            assert "count_reads_fast" not in err
        else:
            assert "count_reads_fast" in err and "handed the call back" not in err, err[-2000:]
            assert ("by counting first" if entry != "dev-full-sort" else "by the full sort") in err
    finally:
        store.close()


# ---------------------------------------------------------------------------------------------------------------- extreme counts
C_LO, C_MID, C_HI = 65535, 65536, 65537


def genome_records(k, seed=61):
    """two records of ~1.5 Mbp each: random sequence with runs of N, a poly-A run that gives A^k 65537 occurrences, a poly-C run that gives
    C^k 65536, and an (AC) repeat whose two phases occur 65535 times each (every run between letters that end it)"""
    rng = np.random.default_rng(seed)

    def rnd(n):
        s = rng.choice(list("ACGT"), size=n)
        for at in range(50_000, n - 1000, 200_000):
            s[at:at + int(rng.integers(1, 600))] = "N"
        return "".join(s)

    a = rnd(1_400_000)
    b = rnd(1_500_000)
    r1 = a[:700_000] + "C" + "A" * (C_HI + k - 1) + "C" + a[700_000:] + "G" + "AC" * ((2 * C_LO + k) // 2) + "ACA"[: (2 * C_LO + k) % 2] + "G"
    r2 = b[:900_000] + "A" + "C" * (C_MID + k - 1) + "A" + b[900_000:]
    return [r1, "ACGT" * 40, r2]


_XDATA = {}


def extreme_expect(k, P_):
    if k not in _XDATA:
        m = 10
        reads = genome_records(k)
        lut, rep = orc.minimizer_lut(m), orc.repart_static(m, P_)
        exp = orc.superk_partition(reads, k, m, lut, rep, P_)
        kcounts = [orc.count_kmer(exp[p][0], k, 1) for p in range(P_)]
        allc = np.concatenate([c for _, c in kcounts])
        for c in (C_LO, C_MID, C_HI):
            assert c in set(allc.tolist()), c
        _XDATA[k] = (reads, m, rep, exp, kcounts, orc.superk_stats(reads, k, m, lut, rep, P_))
    return _XDATA[k]


@pytest.mark.parametrize("path", ["waves", "lds-hash", "library"])
@pytest.mark.parametrize("k", [31, 32, 63, 96, 127])
def test_extreme_counts_on_genome_records(ctx, monkeypatch, k, path):
    """counts of 65535, 65536 and 65537 on megabase records: k-mers and window hashes (window 2^40) through kmx_count_batch with each bucket
    path, hard-min at 65536 and at 1; the abundance histogram's upper out-of-range fields exact; kmx_count_reads_dev's device-store records
    read back and its PartiInfo<5> statistics against the oracle's"""
    from kmtricks_amd import lib
    if k >= 64 and path == "lds-hash":
        pytest.skip("keys of three and four words have one bucket path")
    if path == "library":
        monkeypatch.setenv("KMX_COUNT_SORT", "library")
    if path == "lds-hash":
        monkeypatch.setenv("KMX_COUNT_BUCKETS", "hash")
    P_ = 8
    reads, m, rep, exp, kcounts, (epin, ems, emk, _) = extreme_expect(k, P_)
    streams = [e[0] for e in exp]
    W = 1 << 40
    for hm in (C_MID, 1):
        got = ctx.count_batch(streams, k, hm)
        for p in range(P_):
            ek, ec = kcounts[p]
            keep = ec >= hm
            assert np.array_equal(got[p][0], ek[keep]) and np.array_equal(got[p][1], ec[keep]), (hm, p)
        goth = ctx.count_batch(streams, k, hm, window=W, partitions=list(range(P_)))
        for p in range(P_):
            ek, ec = orc.count_hash(streams[p], k, W, p, hm)
            assert np.array_equal(goth[p][0], ek) and np.array_equal(goth[p][1], ec), (hm, p)
    assert sum(len(g[1]) for g in goth) > 2_000_000
    # the histogram of the k-mer counts: the three k-mers beyond its bins (and the (AC) repeat's second phase) in oob[1] / oob[3]
    eh = None
    for _, c in kcounts:
        eh = orc.khist(c, 1, 255, acc=eh)
    assert int(eh["oob"][1]) >= 4 and int(eh["oob"][3]) >= C_LO * 2 + C_MID + C_HI
    ctx.hist_reset()
    ctx.count_batch(streams, k, C_MID)
    h = ctx.hist_read(1, 255)
    ctx.hist_off()
    assert h["oob"].tolist() == eh["oob"].tolist() and h["sums"].tolist() == eh["sums"].tolist()
    assert np.array_equal(h["unique"], eh["unique"]) and np.array_equal(h["total"], eh["total"])
    if path != "waves":
        return
    # split + count into a device store, hard-min at the boundary; statistics far beyond 3 kb records
    store = lib.Store(0)
    try:
        kw = (k + 31) // 32
        for window, hm in ((0, C_MID), (W, C_MID), (0, 1)):
            lists, nk, raw = ctx.count_reads_dev(reads, k, m, rep, P_, hm, [store], window=window, raw=True, sparse=True)
            assert nk == [e[1] for e in exp]
            for p in range(P_):
                gk, gc = ctx.read_list(lists[p][0], lists[p][1], 1 if window else kw)
                ek, ec = orc.count_hash(streams[p], k, W, p, hm) if window else orc.count_kmer(streams[p], k, hm)
                assert np.array_equal(gk.reshape(ek.shape), ek) and np.array_equal(gc, ec), (window, hm, p)
            pr, ms, mk, nsk = raw
            pr = pr.reshape(P_, 5, 256).astype(np.uint64)
            assert np.array_equal(pr.reshape(P_, 1280), epin[:, 2:]) and np.array_equal(ms, ems) and np.array_equal(mk, emk) and nsk == int(ems.sum())
    finally:
        store.close()


def test_count_beyond_2_to_the_24(ctx):
    """one k-mer counted 2^24 + 3 times (a 16.8 Mbp poly-A record beside random reads): its partition is beyond the sample sort, so the
    library sort and the two-walk path take it -- k-mer and hash counts, the histogram's upper fields, the device store's records"""
    from kmtricks_amd import lib
    k, m, P_ = 31, 10, 4
    n = (1 << 24) + 3
    reads = random_reads(77, 2000, 150) + ["C" + "A" * (n + k - 1) + "C"]
    lut, rep = orc.minimizer_lut(m), orc.repart_static(m, P_)
    exp = orc.superk_partition(reads, k, m, lut, rep, P_)
    streams = [e[0] for e in exp]
    kc = [orc.count_kmer(s, k, 1) for s in streams]
    assert max(int(c.max()) for _, c in kc if len(c)) == n
    ctx.hist_reset()
    got = ctx.count_batch(streams, k, 1)
    h = ctx.hist_read(1, 255)
    ctx.hist_off()
    eh = None
    for p in range(P_):
        assert np.array_equal(got[p][0], kc[p][0]) and np.array_equal(got[p][1], kc[p][1])
        eh = orc.khist(kc[p][1], 1, 255, acc=eh)
    assert h["oob"].tolist() == eh["oob"].tolist() and int(h["oob"][3]) >= n and h["sums"].tolist() == eh["sums"].tolist()
    W = 1 << 40
    goth = ctx.count_batch(streams, k, 2, window=W, partitions=list(range(P_)))
    store = lib.Store(0)
    try:
        lists, nk, _ = ctx.count_reads_dev(reads, k, m, rep, P_, C_MID, [store])
        for p in range(P_):
            ek, ec = orc.count_hash(streams[p], k, W, p, 2)
            assert np.array_equal(goth[p][0], ek) and np.array_equal(goth[p][1], ec)
            gk, gc = ctx.read_list(lists[p][0], lists[p][1], 1)
            keep = kc[p][1] >= C_MID
            assert np.array_equal(gk.reshape(-1), kc[p][0].reshape(-1)[keep]) and np.array_equal(gc, kc[p][1][keep])
    finally:
        store.close()


def test_count_fuzzers_with_wide_windows():
    """scripts/fuzz_count.py --wide and scripts/stress_count.py wide: about half of their random cases draw a window of tests/synth.py's
    shapes"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "fuzz_count.py"), "--cases", "16", "--seed", "5", "--wide"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and '"all_equal_to_oracle": true' in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    assert '"wide_cases": 0' not in r.stdout
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "stress_count.py"), "12", "5", "wide"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all 12 cases equal the oracle" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    assert "window=" in r.stdout
