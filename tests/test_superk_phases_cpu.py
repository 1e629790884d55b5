"""The inputs of the super-k-mer phase sweep, checked without a device: the grid of (k, m) pairs holds every window width
the split kernels can be given; every pair's batch brings each event of the split to every lane of a chunk -- judged by the string
restatement alone (tests/superk_ref.py) --; the restatement and the oracle agree on every batch, byte for byte and counter for counter; and
three deliberately wrong restatements (a window one m-mer short, maxs + 1, a minimizer cut forgotten on a chunk's first lane) differ from
the oracle on every batch: the batches tell width, length and phase mistakes apart.  tests/test_superk_phases_gpu.py runs them."""
import numpy as np
import pytest

import orc
import superk_ref as sr
from synth import superk_record

IDS = [f"k{k}-m{m}" for k, m in sr.PAIRS]
_ORACLE = {}


def parts_of(m):
    return 5 if m <= 11 else 3


def oracle(k, m):
    """(streams + k-mers per partition, statistics or None) of the pair's batch; the last pair's is kept"""
    if (k, m) not in _ORACLE:
        _ORACLE.clear()
        P = parts_of(m)
        lut, rep = orc.minimizer_lut(m), orc.repart_static(m, P)
        reads = sr.phase_batch(k, sr.seed_of(k, m))
        exp = orc.superk_partition(reads, k, m, lut, rep, P)
        _ORACLE[(k, m)] = (reads, rep, exp, orc.superk_stats(reads, k, m, lut, rep, P) if m <= 11 else None)
    return _ORACLE[(k, m)]


def test_the_grid_holds_every_width():
    narrow = {k - m + 1 for k, m in sr.PAIRS if k <= 63}
    wide = {k - m + 1 for k, m in sr.PAIRS if k >= 64}
    assert narrow == set(range(1, 61)) and wide == set(range(50, 125))
    for nbm in (1, 31, 32, 33, 60):           # k == m; the last narrow widths (own = 33, 32); the first wide one; the largest for k <= 63
        assert nbm in narrow, nbm
    for nbm in (50, 63, 64, 65, 124):         # k_superk_wide: the smallest; around its two spans of 64 (the arm of its own at 64); the largest
        assert nbm in wide, nbm
    assert all(8 <= k <= 127 and 4 <= m <= 15 and m <= k for k, m in sr.PAIRS) and len(set(sr.PAIRS)) == len(sr.PAIRS)
    assert {(k, m) for k in (8, 15, 31, 32, 63, 64, 95, 96, 127) for m in (4, 10) if m <= k} <= set(sr.PAIRS)
    assert {(64, m) for m in range(11, 16)} <= set(sr.PAIRS) and {(41, 10), (42, 10)} <= set(sr.PAIRS)
    assert [sr.own_of(k, m) for k, m in ((41, 10), (42, 10), (40, 10), (10, 10), (63, 4), (64, 15), (127, 4))] == [32, 63, 33, 63, 63, 63, 63]
    assert [sr.maxs_of(k) for k in (8, 31, 32, 63, 64, 95, 96, 127)] == [28, 28, 60, 60, 92, 92, 124, 124]


def test_the_batch_is_what_the_sweep_describes():
    k = 31
    reads = sr.phase_batch(k, 5)
    assert len(reads) == 70 and reads == sr.phase_batch(k, 5) and reads != sr.phase_batch(k, 6)
    base = reads[0]
    assert len(base) == 70 + (k + 28 + 8) + 40 + 1 + (k + 50) and base.count("N") == 1 and "A" * (k + 36) in base
    assert all(len(reads[j]) == len(base) + j and reads[j].endswith(base) and reads[63].endswith(reads[j]) for j in range(64))
    assert [len(r) for r in reads[64:68]] == [0, k - 1, k, k] and reads[67] == "T" * k and reads[68] == "ACGTN" * 40
    assert reads[69].islower() and len(reads[69]) > k
    assert sr.record("0123012", 4) == superk_record("ACTGACT", 4) and sr.record("3210", 4) == superk_record("GTCA", 4)


@pytest.mark.parametrize("k,m", sr.PAIRS, ids=IDS)
def test_every_event_reaches_every_lane(k, m):
    """from the restatement alone: each of the six events lies, somewhere in the batch, at every position modulo the chunk's owned positions"""
    own = sr.own_of(k, m)
    seen = {e: set() for e in sr.EVENTS}
    cache = {}
    for read in sr.phase_batch(k, sr.seed_of(k, m)):
        for e, pos in sr.events(sr.superkmers(read, k, m, _cache=cache)):
            seen[e].add(pos % own)
    for e in sr.EVENTS:
        assert seen[e] == set(range(own)), (e, own, sorted(set(range(own)) - seen[e]))


@pytest.mark.parametrize("k,m", sr.PAIRS, ids=IDS)
def test_restatement_against_oracle(k, m):
    reads, rep, exp, stats = oracle(k, m)
    P = parts_of(m)
    got = sr.Split(reads, k, m, rep, P)
    assert sum(got.nk) > 10000
    for p in range(P):
        assert bytes(got.streams[p]) == exp[p][0], p
    assert got.nk == [e[1] for e in exp]
    if stats is not None:
        epin, ems, emk, emx = stats
        assert np.array_equal(got.pinfo_array(), epin)
        for which, e in (("ms", ems), ("mk", emk), ("mx", emx)):
            assert np.array_equal(got.table(which), e), which
        assert [len(s) for s in got.sks if s] and sum(len(s) for s in got.sks) == sum(e[2] for e in exp)


@pytest.mark.parametrize("wrong", sr.WRONG)
@pytest.mark.parametrize("k,m", sr.PAIRS, ids=IDS)
def test_wrong_variants_differ_from_the_oracle(k, m, wrong):
    """a window one m-mer short, a super-k-mer one k-mer too long, a minimizer cut forgotten behind a chunk's first lane: the oracle's streams
    are not theirs, for any pair (the third: such a cut exists in every batch, test_every_event_reaches_every_lane)"""
    reads, rep, exp, _ = oracle(k, m)
    P = parts_of(m)
    bad = sr.Split(reads, k, m, rep, P, wrong=wrong)
    assert [bytes(s) for s in bad.streams] != [e[0] for e in exp]
