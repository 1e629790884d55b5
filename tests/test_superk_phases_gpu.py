"""The super-k-mer split (k_superk_wave, k_superk_wide: superk.hip) at every window width and chunk phase: one case per (k, m)
of superk_ref.PAIRS -- every nbm = k - m + 1 of 1 .. 60 for k <= 63 and of 50 .. 124 for k >= 64 --, its input the pair's phase batch: 64
shifted copies of one read, so that each event of the split (minimizer change, invalid k-mer, the maxs cut, the end of the read, a strand
change, the cut of a strand run at 5) lies on every lane of a chunk, the last owned one and the look-ahead lane included
(tests/test_superk_phases_cpu.py holds that condition).  Every road a read can take through the two kernels is run on the batch:
  * streams: kmx_superk_partition by count + scan + emit, and (k < 64) by the one-pass look-back road;
  * statistics (m <= 11): kmx_superk_partition_stats as it is, with KMX_STATS_ATOMICS=1, and the statistics-only pass (all three count
    kx-mers per minimizer, which only the walk with atomics does: k_superk_wave / k_superk_wide <.., STATS>, streams emitted or not);
  * sync-free count (k < 64, m <= 11): kmx_count_reads_dev with the raw tables in sparse form -- the one-walk road, k_superk_wave<.., CH>,
    which the trace must show was not handed back --, then the same call on the two-walk road (KMX_COUNT_FAST=0: k_superk_wave<.., DEFER>,
    whose strand words k_part_stats counts).
The two one-walk roads size their arrays before they know the data; where the whole batch is more than they take, its reads go in several
calls (one_walk_calls), so that every read still takes them.
Expected values are the oracle's; the string restatement's are compared as well (m <= 11), so that a difference says which of the three
stands alone.  All outputs are integers and bytes: everything is compared exactly."""
import numpy as np
import pytest

import count_shapes as cs
import orc
import superk_ref as sr

pytestmark = pytest.mark.gpu

IDS = [f"k{k}-m{m}" for k, m in sr.PAIRS]
GROUP = 4               # reads a call where the whole batch holds more records than the one-walk roads take (below)
CS_CAP_U128 = 4096      # count_sort.hpp, CsCap<__uint128_t>::cap: 128-bit keys of a bucket
_TABLES = {}


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def parts_of(m):
    return 5 if m <= 11 else 3


def tables(m):
    """(minimizer look-up table of the oracle, static repartition) -- the last m's are kept (m = 15: 6 GiB)"""
    if m not in _TABLES:
        _TABLES.clear()
        _TABLES[m] = (orc.minimizer_lut(m), orc.repart_static(m, parts_of(m)))
    return _TABLES[m]


class Want:
    """what the oracle (and, m <= 11, the restatement) say of `reads`"""

    def __init__(self, reads, k, m):
        from kmtricks_amd import lib
        lut, rep = tables(m)
        P = parts_of(m)
        self.reads, self.packed, self.P = reads, lib.Context.pack_reads(reads), P
        exp = orc.superk_partition(reads, k, m, lut, rep, P)
        self.streams, self.nk, self.nd = [e[0] for e in exp], [int(e[1]) for e in exp], sum(int(e[2]) for e in exp)
        self.stats = self.ref = None
        if m <= 11:
            self.stats = orc.superk_stats(reads, k, m, lut, rep, P)
            self.ref = sr.Split(reads, k, m, rep, P)
            self.ref_stats = (self.ref.pinfo_array(), self.ref.table("ms"), self.ref.table("mk"), self.ref.table("mx"))


def same(what, got, oracle, ref=None):
    """got == oracle (== ref); a failure names the one that stands alone"""
    def eq(a, b):
        return np.array_equal(a, b) if isinstance(a, np.ndarray) or isinstance(b, np.ndarray) else a == b
    if eq(got, oracle) and (ref is None or eq(ref, oracle)):
        return
    if ref is None:
        who = "the device and the oracle differ (no restatement at this m)"
    elif eq(ref, oracle):
        who = "the device stands alone: oracle and restatement agree"
    elif eq(got, ref):
        who = "the oracle stands alone: device and restatement agree"
    elif eq(got, oracle):
        who = "the restatement stands alone: device and oracle agree"
    else:
        who = "all three differ"
    where = ""
    if isinstance(got, list) and isinstance(oracle, list):
        where = f"; first at index {next((i for i, (a, b) in enumerate(zip(got, oracle)) if not eq(a, b)), None)}"
    pytest.fail(f"{what}: {who}{where}")


def check_streams(what, got, w):
    same(what + ": streams", [g[0] for g in got], w.streams, w.ref and [bytes(s) for s in w.ref.streams])
    same(what + ": k-mers per partition", [g[1] for g in got], w.nk, w.ref and w.ref.nk)


def check_stats(what, pin, ms, mk, mx, w):
    for name, g, o, r in zip(("PartiInfo", "super-k-mers per minimizer", "k-mers per minimizer", "kx-mers per minimizer"), (pin, ms, mk, mx), w.stats, w.ref_stats):
        same(f"{what}: {name}", g, o, r)


def check_count(ctx, what, w, k, m, rep, capfd, fast):
    """kmx_count_reads_dev into one store at hard-min 1, the raw tables in sparse form; fast: the trace must show the one-walk road, not handed back"""
    from kmtricks_amd import lib
    kw = orc.kw_of_k(k)
    store = lib.Store(0)
    try:
        capfd.readouterr()
        lists, nk, raw = ctx.count_reads_dev(w.packed, k, m, rep, w.P, 1, [store], raw=True, sparse=True)
        err = capfd.readouterr().err
        got = [ctx.read_list(lists[p][0], lists[p][1], kw) for p in range(w.P)]
    finally:
        store.close()
    if fast:
        tr = cs.trace_fast(err)
        assert len(tr) == 1 and cs.HANDED_BACK not in err, (what, err[-1500:])
        assert (tr[0]["records"], tr[0]["kmers"], tr[0]["status"], tr[0]["overflow"]) == (w.nd, sum(w.nk), 0, 0), (what, tr[0], w.nd)
    else:
        assert "count_reads_fast" not in err and cs.HANDED_BACK not in err, (what, err[-1500:])
    same(what + ": k-mers per partition", nk, w.nk, w.ref.nk)
    for p in range(w.P):
        ek, ec = orc.count_kmer(w.streams[p], k, 1)
        rk, rc = orc.count_kmer(bytes(w.ref.streams[p]), k, 1)
        same(f"{what}: keys of partition {p}", np.asarray(got[p][0]).reshape(-1, kw), ek.reshape(-1, kw), rk.reshape(-1, kw))
        same(f"{what}: counts of partition {p}", got[p][1], ec, rc)
    pr, ms, mk, nsk = raw
    same(what + ": raw PartiInfo", pr.reshape(w.P, 1280).astype(np.uint64), w.stats[0][:, 2:], w.ref_stats[0][:, 2:])
    same(what + ": raw super-k-mers per minimizer", ms.astype(np.uint64), w.stats[1], w.ref_stats[1])
    same(what + ": raw k-mers per minimizer", mk.astype(np.uint64), w.stats[2], w.ref_stats[2])
    same(what + ": super-k-mers", nsk, w.nd, sum(len(s) for s in w.ref.sks))


def one_walk_calls(whole, k, m):
    """the batch as the calls of the one-walk roads take it.  Both size their descriptor arrays before the walk: the sync-free count for
    bases / 4 + reads + 1024 records (count_shapes.plan), the look-back split for k-mers / 2 + reads + 1024; a batch with more is sent the
    two-walk way, by design.  At nbm <= 5 or so a super-k-mer holds too few k-mers for the whole batch to fit: its reads then go GROUP a
    call, which fit thanks to the 1024.  And the count behind the sync-free split sorts 128-bit keys (k = 33 .. 63) in buckets of at most
    CS_CAP_U128 k-mers, equal ones cannot be parted, and the batch holds its all-A k-mer 64 x (maxs + 9) = 4416 times: such a sample is
    handed to the library sort, by design again; the batch then goes in two calls of 35 reads.  Every read still takes the road, and the
    test insists that every call stayed on it."""
    kw = orc.kw_of_k(k)
    poly_a = sr.maxs_of(k) + 9      # all-A k-mers of a shifted read
    if whole.nd > cs.plan(len(whole.reads), len(whole.packed[0]), whole.P, kw)["nd_cap"]:
        size = GROUP
    elif kw == 2 and 64 * poly_a + 1 > CS_CAP_U128:
        size = 35
    else:
        return [whole]
    calls = [Want(whole.reads[a:a + size], k, m) for a in range(0, len(whole.reads), size)]
    for c in calls:
        assert c.nd <= cs.plan(len(c.reads), len(c.packed[0]), c.P, kw)["nd_cap"], (k, m, c.nd)
        assert kw == 1 or len(c.reads) * poly_a + 1 <= CS_CAP_U128
    return calls


@pytest.mark.parametrize("k,m", sr.PAIRS, ids=IDS)
def test_split_at_every_width_and_phase(ctx, k, m, monkeypatch, capfd):
    _, rep = tables(m)
    P = parts_of(m)
    w = Want(sr.phase_batch(k, sr.seed_of(k, m)), k, m)
    assert sum(w.nk) > 10000
    calls = one_walk_calls(w, k, m) if k < 64 and m <= 11 else [w]
    # ---- streams and k-mers per partition
    check_streams("two passes", ctx.superk_partition(w.packed, k, m, rep, P), w)
    if k < 64:
        monkeypatch.setenv("KMX_SUPERK_ONE_PASS", "1")
        for i, c in enumerate(calls):
            check_streams(f"look-back, call {i}", ctx.superk_partition(c.packed, k, m, rep, P), c)
        monkeypatch.delenv("KMX_SUPERK_ONE_PASS")
    if m > 11:
        return
    # ---- statistics
    got, pin, ms, mk, mx = ctx.superk_partition_stats(w.packed, k, m, rep, P)
    check_streams("statistics", got, w)
    check_stats("statistics", pin, ms, mk, mx, w)
    monkeypatch.setenv("KMX_STATS_ATOMICS", "1")
    got, pin, ms, mk, mx = ctx.superk_partition_stats(w.packed, k, m, rep, P)
    monkeypatch.delenv("KMX_STATS_ATOMICS")
    check_streams("statistics by atomics", got, w)
    check_stats("statistics by atomics", pin, ms, mk, mx, w)
    none, pin, ms, mk, mx = ctx.superk_partition_stats(w.packed, k, m, rep, P, streams=False)
    assert none is None
    check_stats("statistics only", pin, ms, mk, mx, w)
    if k >= 64:
        return
    # ---- the sync-free count, then the two-walk road
    monkeypatch.setenv("KMX_TRACE", "1")
    for i, c in enumerate(calls):
        check_count(ctx, f"sync-free count, call {i}", c, k, m, rep, capfd, fast=True)
    monkeypatch.setenv("KMX_COUNT_FAST", "0")
    check_count(ctx, "two-walk count", w, k, m, rep, capfd, fast=False)
