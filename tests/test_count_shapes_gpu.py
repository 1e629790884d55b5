"""kmx_count_reads_dev's sync-free path at every grid a whole sample gives it.  Every launch shape on that path
is computed from the data, so the cases of tests/count_shapes.py are inputs: reads and partitions for the split's grids (k_superk_wave<.., CH>,
k_sk_hist, k_sk_scan, k_sk_scatter), k-mers of ONE partition to the unit for the sample sort's layout (k_superk_decode_kmers, k_cs_splitters,
k_cs_walk, k_cs_scatter_staged, the bucket kernels), buckets to the unit for k_cs_scan_mw's carry across workgroups.  Each case is compared
with (a) the oracle -- lists, k-mers per partition, PartiInfo and per-minimizer tables --, (b) the same call on the two-walk path
(KMX_COUNT_FAST=0), and (c) the trace: the `[kmx count_reads_plan]` line must state the grid the case aims at, the `[kmx count_reads_fast]`
line the real buckets and walk chunks the oracle's k-mers give.  A case that does not run its shape fails."""
import numpy as np
import pytest

import count_shapes as cs
import orc

pytestmark = pytest.mark.gpu

PARAMS = [(c.id, mode) for c in cs.CASES.values() for mode in c.modes]
SKF_ST_LAYOUT = 4      # skf.hpp: a partition beyond the sample sort's limits

_WANT = {}


def want(d, case_id, hashed, hard_min):
    """the oracle's lists of the case: [(keys, counts)] per partition; kept for the case's modes"""
    key = (case_id, hashed, hard_min)
    if key not in _WANT:
        if not any(k_[0] == case_id for k_ in _WANT):
            _WANT.clear()
        _WANT[key] = [orc.count_hash(d.exp[p][0], d.k, cs.W_HASH, p, hard_min) if hashed else orc.count_kmer(d.exp[p][0], d.k, hard_min) for p in range(d.P)]
    return _WANT[key]


def same_lists(got, exp, what):
    assert len(got) == len(exp)
    for p, ((gk, gc), (ek, ec)) in enumerate(zip(got, exp)):
        assert len(gc) == len(ec) and np.array_equal(np.asarray(gk).reshape(np.asarray(ek).shape), ek) and np.array_equal(gc, ec), (what, p, len(gc), len(ec))


def same_tables(raw, d, what):
    pr, ms, mk, nsk = raw
    assert np.array_equal(pr.reshape(d.P, 1280).astype(np.uint64), d.pinfo[:, 2:]), what
    assert np.array_equal(ms, d.ms) and np.array_equal(mk, d.mk) and nsk == d.nd, what


def check_trace(err, case, d, mode):
    """(c): the path that ran, the grid the host planned, the sizes the device found"""
    plans, fast = cs.trace_plans(err), cs.trace_fast(err)
    if not case.fast:
        assert not plans and "count_reads_fast" not in err and cs.HANDED_BACK not in err, err[-2000:]
        return
    assert len(plans) == 1 and len(fast) == 1, err[-2000:]
    p = d.plan(mode)
    assert plans[0] == {k: p[k] for k in cs.PLAN_KEYS}, (plans[0], p)
    kw = d.key_words(mode)
    real = dict(TB=cs.buckets(d.nk), NC=cs.walk_chunks(d.nk, kw), kmers=sum(d.nk))
    for key, aim in d.aim.items():      # the shape the case is there for, as the call itself reports it
        if key in plans[0]:
            assert plans[0][key] == aim, (key, plans[0][key], aim)
        elif key in real:
            assert fast[0][key] == aim == real[key], (key, fast[0][key], aim, real[key])
    if case.handback:
        assert err.count(cs.HANDED_BACK) == 1 and fast[0]["status"] == SKF_ST_LAYOUT, err[-2000:]
        return
    assert cs.HANDED_BACK not in err, err[-2000:]
    assert (fast[0]["records"], fast[0]["kmers"], fast[0]["TB"], fast[0]["NC"]) == (d.nd, real["kmers"], real["TB"], real["NC"]), (fast[0], d.nd, real)
    assert fast[0]["status"] == 0 and fast[0]["overflow"] == 0
    assert fast[0]["road"] == ("by the full sort" if kw == 2 or mode.endswith("-sort") else "by counting first")


@pytest.mark.parametrize("case_id,mode", PARAMS)
def test_sync_free_count_at_every_grid(case_id, mode, monkeypatch, capfd):
    from kmtricks_amd import lib
    case, d = cs.CASES[case_id], cs.data(case_id)
    hashed = mode.startswith("hashed")
    kw = d.key_words(mode)
    monkeypatch.setenv("KMX_TRACE", "1")
    monkeypatch.setenv("KMX_COUNT_HASH_FIRST", "0" if mode.endswith("-sort") else "1")      # (the road pinned: not the last call's lost buckets)
    ctx = lib.Context(0)      # (a fresh context: no estimate of an earlier case decides how the lists are packed)

    def call(hard_min, **kwargs):
        store = lib.Store(0)
        try:
            capfd.readouterr()
            lists, nk, raw = ctx.count_reads_dev(d.packed, d.k, d.m, d.rep, d.P, hard_min, [store], window=cs.W_HASH if hashed else 0, **kwargs)
            got = [ctx.read_list(lists[p][0], lists[p][1], kw) for p in range(d.P)]
            return got, nk, raw, capfd.readouterr().err
        finally:
            store.close()

    try:
        # the sync-free call, the statistics per partition (k_part_stats); the context's first call: the lists are packed once their sizes are known
        got, nk, raw, err = call(2, raw=True, sparse=True)
        check_trace(err, case, d, mode)
        assert nk == d.nk
        same_lists(got, want(d, case_id, hashed, 2), "sync-free, hard-min 2")
        same_tables(raw, d, "sync-free, sparse tables")
        for p in range(d.P):      # (empty partitions -- 1024 partitions over 4^7 minimizers, the trailing ones of the bucket-scan cases -- give empty lists)
            assert d.nk[p] or len(got[p][1]) == 0
        if "empty_tail" in d.aim:
            assert all(n == 0 for n in nk[d.P - d.aim["empty_tail"]:]) and all(n > 0 for n in nk[:cs.SCAN_Q])
        # again with hard-min 1: the lists go into room reserved from the first call's estimate (k_cs_compact_recs)
        got1, nk1, _, err1 = call(1)
        check_trace(err1, case, d, mode)
        assert nk1 == d.nk
        same_lists(got1, want(d, case_id, hashed, 1), "sync-free, hard-min 1")
        # (b) the two-walk path: the same bytes
        monkeypatch.setenv("KMX_COUNT_FAST", "0")
        got_b, nk_b, raw_b, err_b = call(2, raw=True, sparse=True)
        monkeypatch.delenv("KMX_COUNT_FAST")
        assert "count_reads_plan" not in err_b and "count_reads_fast" not in err_b
        assert nk_b == nk
        for p in range(d.P):
            assert got_b[p][0].tobytes() == got[p][0].tobytes() and got_b[p][1].tobytes() == got[p][1].tobytes(), p
        for a, b in zip(raw_b[:3], raw[:3]):
            assert a.tobytes() == b.tobytes()
        assert raw_b[3] == raw[3]
        # the dense form of the tables (counted while the reads are walked)
        got_d, nk_d, raw_d, _ = call(2, raw=True)
        assert nk_d == d.nk
        same_lists(got_d, want(d, case_id, hashed, 2), "dense tables")
        same_tables(raw_d, d, "dense tables")
    finally:
        ctx.close()
