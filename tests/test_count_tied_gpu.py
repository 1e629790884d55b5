"""Every count entry point on k-mers that tie in their leading words (tests/tied_reads.py: the final order, the bucket and every run boundary
decided by a key's LOWER words; the tied group of a wide key one bucket of each size class, up to the overflow that hands the batch to the
library's radix passes; the bucket look-up table's corners), keys and counts exactly the oracle's at hard-min 1 and 2."""
import numpy as np
import pytest

import orc
import tied_reads as T
from test_count_keyspace_gpu import ctx      # noqa: F401 (the module's context fixture)

pytestmark = pytest.mark.gpu

P, M = T.P, T.M
IDS = [c["id"] for c in T.CASES]
_WANT = {}


def _same(got, exp, what):
    for p in range(P):
        (gk, gc), (ek, ec) = got[p], exp[p]
        assert np.array_equal(np.asarray(gk).reshape(ek.shape), ek) and np.array_equal(gc, ec), (what, p, len(gc), len(ec))


def want(case, hard_min):
    key = (case["id"], hard_min)
    if key not in _WANT:
        _WANT[key] = [orc.count_kmer(s[0], case["k"], hard_min) for s in T.batch(case)[2]]
    return _WANT[key]


BATCH_PATHS = [(c, p) for c in T.CASES for p in ("waves", "library", "lds-hash", "lds-sort") if c["k"] <= 64 or not p.startswith("lds-")]


@pytest.mark.parametrize("case,path", BATCH_PATHS, ids=[f"{c['id']}-{p}" for c, p in BATCH_PATHS])
def test_count_batch_on_tied_kmers(ctx, monkeypatch, case, path):
    """kmx_count_batch: the sample sort with the wave kernels and the LDS kernels behind them (a wide key's tied group beyond CsCap::cap:
    the overflow word, then wide_sort_count), the library sort forced (KMX_COUNT_SORT=library), one- and two-word keys with every bucket by
    the LDS hash set or the LDS sort (KMX_COUNT_BUCKETS=hash|sort)"""
    if path == "library":
        monkeypatch.setenv("KMX_COUNT_SORT", "library")
    if path.startswith("lds-"):
        monkeypatch.setenv("KMX_COUNT_BUCKETS", path[4:])
    streams = [s[0] for s in T.batch(case)[2]]
    for hard_min in (1, 2):
        _same(ctx.count_batch(streams, case["k"], hard_min), want(case, hard_min), (path, hard_min))


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_count_reads_on_tied_kmers(ctx, case):
    """kmx_count_reads, the streams handed back: the split's records and the counts"""
    reads, rep, exp, _ = T.batch(case)
    for hard_min in (1, 2):
        got, nk, streams, _ = ctx.count_reads(reads, case["k"], M, rep, P, hard_min, streams=True)
        assert nk == [e[1] for e in exp] and streams == [e[0] for e in exp]
        _same(got, want(case, hard_min), ("kmx_count_reads", hard_min))


DEV_ENTRIES = [(c, e) for c in T.CASES for e in ("counting-first", "full-sort", "no-table", "two-walks") if c["k"] < 64 or e == "two-walks"]


@pytest.mark.parametrize("case,entry", DEV_ENTRIES, ids=[f"{c['id']}-{e}" for c, e in DEV_ENTRIES])
def test_count_reads_dev_on_tied_kmers(ctx, monkeypatch, capfd, case, entry):
    """kmx_count_reads_dev, the records read back from the device store.  k < 64: the sync-free path -- counting first (one-word keys: k_cs_wave_count),
    the full sort, without the bucket look-up table (KMX_COUNT_LUT=0).  The splitters of one- and two-word keys are whole keys, so a tied
    group is cut into buckets like any other keys and no case reaches the path's bucket limit (4096 keys): KMX_TRACE must not name a
    hand-back.  All k: the two-walk path (KMX_COUNT_FAST=0)."""
    from kmtricks_amd import lib
    reads, rep, exp, _ = T.batch(case)
    k, kw = case["k"], orc.kw_of_k(case["k"])
    monkeypatch.setenv("KMX_TRACE", "1")
    monkeypatch.setenv("KMX_COUNT_HASH_FIRST", "1" if entry == "counting-first" else "0")
    if entry == "no-table":
        monkeypatch.setenv("KMX_COUNT_LUT", "0")
    if entry == "two-walks":
        monkeypatch.setenv("KMX_COUNT_FAST", "0")
    store = lib.Store(0)
    try:
        for hard_min in (1, 2):
            capfd.readouterr()
            lists, nk, _ = ctx.count_reads_dev(reads, k, M, rep, P, hard_min, [store])
            err = capfd.readouterr().err
            assert nk == [e[1] for e in exp]
            _same([ctx.read_list(lists[p][0], lists[p][1], kw) for p in range(P)], want(case, hard_min), (entry, hard_min))
            if entry == "two-walks":
                assert "count_reads_fast" not in err
            else:
                assert "count_reads_fast" in err and "handed the call back" not in err, err[-2000:]
                assert ("by counting first" if entry == "counting-first" and k <= 32 else "by the full sort") in err
    finally:
        store.close()


ABOVE_CAP = [next(c for c in T.CASES if c["cls"] == "above-cap" and T.key_type(c["k"]) == kt) for kt in T.KEY_TYPES]


@pytest.mark.parametrize("case", ABOVE_CAP, ids=[c["id"] for c in ABOVE_CAP])
def test_histogram_on_the_largest_tied_groups(ctx, case):
    """the abundance histogram over a batch whose tied group is beyond CsCap::cap: wide keys give up the sample sort after its bucket kernels
    ran (the histogram of that attempt must not be added) and count by the library passes -- every distinct k-mer once, before hard-min"""
    reads, rep, exp, _ = T.batch(case)
    eh = None
    for _, c in want(case, 1):
        eh = orc.khist(c, 1, 255, acc=eh)
    try:
        ctx.hist_reset()
        ctx.count_batch([e[0] for e in exp], case["k"], 2)
        h = ctx.hist_read(1, 255)
        ctx.hist_reset()
        ctx.count_reads(reads, case["k"], M, rep, P, 3)
        h2 = ctx.hist_read(1, 255)
    finally:
        ctx.hist_off()
    for got in (h, h2):
        assert all(np.array_equal(got[f], eh[f]) for f in ("unique", "total", "oob", "sums")), (got["sums"], eh["sums"])
    assert int(eh["unique"][1]) > 0 and int(eh["unique"][2]) > 0      # (k-mers seen twice and three times)
