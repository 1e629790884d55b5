"""tests/count_shapes.py without a GPU: its constants against skf.hpp / count_sort.hpp / the host code (a constant that moves marks the
shape table stale instead of letting it miss its edges in silence), its builders' exact totals, and every case's aim -- rows, waves a
row, k_sk_scan's workgroups, buckets -- computed from the oracle's split alone, inside the sync-free path's own limits."""
import os
import re

import numpy as np
import pytest

import count_shapes as cs
import orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kmtricks_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_constants_of_the_split_are_the_headers():
    skf = _src("skf.hpp")
    assert int(_one(r"constexpr u32 SKF_RPW = (\d+);", skf)) == cs.SKF_RPW
    assert int(_one(r"constexpr u32 SKF_MAXP = (\d+);", skf)) == cs.SKF_MAXP
    assert int(_one(r"constexpr u32 SKF_DK = (\d+);", skf)) == cs.SKF_DK
    b1, w1, b2, w2, w3 = map(int, _one(r"skf_wpg\(u32 P\) \{ return P <= (\d+) \? (\d+)u : P <= (\d+) \? (\d+)u : (\d+)u; \}", skf))
    assert ((b1, w1), (b2, w2), (cs.SKF_MAXP, w3)) == cs.WPG_STEPS
    for P, w in ((1, 16), (256, 16), (257, 8), (512, 8), (513, 4), (1024, 4)):
        assert cs.skf_wpg(P) == w
    host = _src("superk.hip")
    lo, add, div = map(int, _one(r"rpg = std::max<u32>\((\d+)u, \(R \+ (\d+)u\) / (\d+)u\), Gc = \(R \+ rpg - 1\) / rpg;", host))
    assert (lo, add + 1, div) == (cs.SCAN_MIN_ROWS, cs.SCAN_MAX_WG, cs.SCAN_MAX_WG)
    assert "n_chunks = (u32)((n_seqs + SKF_RPW - 1) / SKF_RPW), R = (n_chunks + wpg - 1) / wpg;" in host
    assert "nd_cap = (u32)std::min<u64>(total_bases, total_bases / 4 + n_seqs + 1024);" in host
    assert "tb_max = (u32)(kb / L.target) + P + 1, nc_max = (u32)(kb / L.chunk) + P + 1, nb_max = (u32)((kb + SKF_DK - 1) / SKF_DK) + 1;" in host
    assert "nb_parts <= SKF_MAXP" in host


def test_constants_of_the_sample_sort_are_the_headers():
    srt = _src("count_sort.hpp")
    assert int(_one(r"constexpr int CS_WALK_TPB = (\d+);", srt)) == cs.CS_WALK_TPB
    assert int(_one(r"constexpr int CS_MAXB = (\d+);", srt)) == cs.CS_MAXB
    assert int(_one(r"cs_target\(\) \{ return (\d+)u; \}", srt)) == cs.CS_TARGET
    g = _one(r"template <typename K> struct CsCap \{ static constexpr int cap = \d+, sample = (\d+), walk = (\d+); \};", srt)
    w = _one(r"template <> struct CsCap<__uint128_t> \{ static constexpr int cap = \d+, sample = (\d+), walk = (\d+); \};", srt)
    assert {1: int(g[0]), 2: int(w[0])} == cs.CS_SAMPLE and {1: int(g[1]), 2: int(w[1])} == cs.CS_WALK
    assert "cs_chunk() { return (u32)CsCap<K>::walk * (u32)CS_WALK_TPB; }" in srt
    assert int(_one(r"cs_schunk\(\) \{ return (\d+)u / \(u32\)sizeof\(K\); \}", srt)) == 65536
    assert (cs.cs_schunk(1), cs.cs_schunk(2), cs.cs_chunk(1), cs.cs_chunk(2)) == (8192, 4096, 16384, 16384)
    assert "static_assert(CS_MAXB == 2 * CS_WALK_TPB" in srt                      # two buckets a thread of k_cs_scatter_staged
    assert int(_one(r"const u32 i = g \* (\d+)u \+ tid \* 4u;", srt)) == cs.CS_SCAN_MW      # k_cs_scan_mw's tile
    cnt = _src("count.hip")
    assert int(_one(r"const dim3 gs\(\(TBm \+ 1 \+ (\d+)\) / (\d+)\);", cnt)[1]) == cs.CS_SCAN_MW
    assert "SkfLayout{cs_target<u64>(), cs_chunk<u64>(), (u32)CS_MAXB, (u32)CsCap<u64>::sample}" in cnt
    # k_sk_scan hands a partition back beyond CS_MAXB buckets or 4 sampled keys a bucket: the first is the tighter one for both key types
    assert "if (nb > L.maxb || nb * 4u > L.sample) bad = true;" in _src("superk_fast.hpp")
    assert all(cs.CS_MAXB * 4 <= s for s in cs.CS_SAMPLE.values())


def test_plan_by_hand():
    """the issue's own arithmetic"""
    p = cs.plan(262145, 4_000_000, 1024, 1)
    assert (p["chunks"], p["rows"], p["wpg"], p["rpg"], p["Gc"], p["pbits"]) == (16385, 4097, 4, 33, 125, 10)
    assert (p["tb_max"], p["nc_max"], p["nb_max"], p["scan_mw"]) == (4_000_000 // 416 + 1025, 4_000_000 // 16384 + 1025, 3908, 3)
    assert cs.plan(8192, 10 ** 5, 256, 1)["Gc"] == 1 and cs.plan(8193, 10 ** 5, 256, 2)["Gc"] == 2
    assert cs.plan(2048, 10 ** 5, 513, 1)["Gc"] == 1 and cs.plan(2049, 10 ** 5, 513, 1)["Gc"] == 2
    assert [cs.plan(100, 1000, P, 1)["pbits"] for P in (1, 2, 3, 4, 5, 256, 257, 1024)] == [1, 1, 2, 2, 3, 8, 9, 10]
    assert cs.buckets([0, 1, 416, 417, 851968]) == 1 + 1 + 1 + 2 + 2048
    assert cs.walk_chunks([0, 1, 16384, 16385], 1) == 0 + 1 + 1 + 2


def test_trace_lines_are_parsed():
    err = ("[kmx count_reads_plan] reads 17 chunks 2 rows 1 wpg 16 Gc 1 rpg 32 pbits 3 tb_max 9 nc_max 9 nb_max 2 scan_mw 1\n"
           "[kmx count_reads_fast] split+decode+sort+count 0.31 ms\n"
           "[kmx count_reads_fast] records 9 k-mers 28 buckets 8 walk chunks 5 listed buckets 0 status 0 overflow 0; the buckets by counting first (0 of them sorted: their distinct keys beyond the table)\n")
    assert cs.trace_plans(err) == [dict(reads=17, chunks=2, rows=1, wpg=16, Gc=1, rpg=32, pbits=3, tb_max=9, nc_max=9, nb_max=2, scan_mw=1)]
    assert cs.trace_fast(err) == [dict(records=9, kmers=28, TB=8, NC=5, listed=0, status=0, overflow=0, road="by counting first")]


@pytest.mark.parametrize("n", [1, 5, 6, 17, 3000])
def test_short_reads(n):
    k = 21
    blob, offs = cs.short_reads(n, k, seed=n)
    reads = cs.reads_list((blob, offs))
    assert len(reads) == n and int(offs[-1]) == len(blob) and set(blob) <= set(b"ACGTN")
    lens = np.diff(offs.astype(np.int64))
    assert lens.min() >= 0 and lens.max() <= k + 11 and lens[0] == k + 11 and b"N" not in reads[0]
    assert cs.short_reads(n, k, seed=n)[0] == blob and (n < 2 or cs.short_reads(n, k, seed=n + 1)[0] != blob)
    if n >= 6:
        assert [len(r) for r in reads[1:6]] == [0, k - 1, k, k + 1, k + 3] and reads[5] == b"N" * (k + 3)
    if n == 3000:
        assert len(set(lens.tolist())) == k + 12                                  # every length from 0 to k + 11
        full = [r for r in reads if len(r) >= k]
        assert 0.15 < 1 - len(set(full)) / len(full) < 0.45                       # copies ...
        assert 20 < sum(b"N" in r for r in reads) < 300                           # ... and reads with an N
        # hard_min = 2 keeps some keys and drops others
        rec = orc.superk_partition(reads, k, 7, orc.minimizer_lut(7), np.zeros(4 ** 7, np.uint16), 1)[0][0]
        c = orc.count_kmer(rec, k, 1)[1]
        assert (c >= 2).sum() > 500 and (c == 1).sum() > 500


@pytest.mark.parametrize("k", [31, 47])
@pytest.mark.parametrize("total", [1, 2, 415, 416, 1024, 8193, 16385])
def test_exact_kmers(total, k):
    packed = cs.exact_kmers(total, k, seed=total)
    reads = cs.reads_list(packed)
    assert all(len(r) >= k and b"N" not in r for r in reads)
    assert sum(len(r) - k + 1 for r in reads) == total
    exp = cs.oracle_split(packed, k, 10, np.zeros(4 ** 10, np.uint16), 1)[0]
    assert exp[0][1] == total
    if total >= 8193:
        assert 0.3 < 1 - len(set(reads)) / len(reads) < 0.7


def test_chunk_of():
    k, m = 21, 7
    lut, one = orc.minimizer_lut(m), np.zeros(4 ** m, np.uint16)
    for d in (0, 1, 63, 64, 65, 129):
        reads = cs.chunk_of(d, k, m)
        assert len(reads) == cs.SKF_RPW and orc.superk_partition(reads, k, m, lut, one, 1)[0][2] == d
        assert cs.chunk_of(d, k, m) == reads


def test_oracle_split_is_the_two_oracle_calls():
    k, m, P = 21, 7, 5
    packed = cs.short_reads(400, k, seed=9)
    lut, rep = orc.minimizer_lut(m), orc.repart_static(m, P)
    exp, pin, ms, mk = cs.oracle_split(packed, k, m, rep, P)
    reads = cs.reads_list(packed)
    assert exp == orc.superk_partition(reads, k, m, lut, rep, P)
    epin, ems, emk, _ = orc.superk_stats(reads, k, m, lut, rep, P)
    assert np.array_equal(pin, epin) and np.array_equal(ms, ems) and np.array_equal(mk, emk)


def test_the_table_holds_every_row_of_the_issue():
    ids = set(cs.CASES)
    for n in (1, 15, 16, 17, 65):
        assert f"reads-{n}" in ids
    for P in (1, 2, 3, 255, 256, 257, 512, 513, 1023, 1024, 1025):
        assert f"parts-{P}" in ids
    assert {"chunk-fill", "chunk-fill-one-partition", "scan-2wg-P1024", "scan-2wg-P256", "scan-3wg-P1024", "scan-125wg-P1024"} <= ids
    common = (1, 415, 416, 417, 1023, 1024, 1025, 16384, 16385, 425984, 425985, 851968, 851969)
    for t in common + (8192, 8193):
        assert cs.CASES[f"sort-u64-{t}"].modes[:1] == ("plain",) and "hashed" in cs.CASES[f"sort-u64-{t}"].modes
    for t in common + (4096, 4097):
        assert f"sort-u128-{t}" in ids
    for t in (425984, 425985):
        assert {"plain", "plain-sort"} <= set(cs.CASES[f"sort-u64-{t}"].modes)
    assert {"buckets-4095", "buckets-4096", "buckets-4097", "buckets-two-carries"} <= ids
    assert [c.id for c in cs.CASES.values() if c.handback] == ["sort-u64-851969", "sort-u128-851969"]
    assert [c.id for c in cs.CASES.values() if not c.fast] == ["parts-1025"]


@pytest.mark.parametrize("case_id", list(cs.CASES))
def test_case_reaches_its_shape_inside_the_paths_limits(case_id):
    """the aim of every case from the oracle alone: the plan's numbers, the real buckets and walk chunks, and the limits that decide
    whether the call stays on the sync-free path -- records <= nd_cap, buckets a partition <= CS_MAXB, the bounds >= the real sizes"""
    case, d = cs.CASES[case_id], cs.data(case_id)
    for mode in case.modes:
        kw = d.key_words(mode)
        p = d.plan(mode)
        tb, nc = cs.buckets(d.nk), cs.walk_chunks(d.nk, kw)
        tail = d.aim.get("empty_tail", 0)      # (the trailing partitions that must be empty)
        got = dict(p, TB=tb, NC=nc, kmers=sum(d.nk), empty_tail=sum(1 for n in d.nk[d.P - tail:] if n == 0))
        for key, want in d.aim.items():
            assert got[key] == want, (key, got[key], want)
        assert sum(d.nk) >= 1 and d.bases < 500 << 20
        if not case.fast:
            assert d.P > cs.SKF_MAXP
            continue
        assert d.P <= cs.SKF_MAXP and d.nd <= p["nd_cap"]
        assert tb <= p["tb_max"] and nc <= p["nc_max"] and cs.ceil_div(sum(d.nk), cs.SKF_DK) <= p["nb_max"] and p["scan_mw"] <= 256
        assert (max(cs.nb_of(n) for n in d.nk) > cs.CS_MAXB) == case.handback
    if case_id == "parts-1024":
        assert any(n == 0 for n in d.nk)
    if case_id == "chunk-fill-one-partition":
        assert [i for i, n in enumerate(d.nk) if n] == [5]
    if case_id == "buckets-two-carries":
        assert cs.buckets(d.nk) > 2 * cs.CS_SCAN_MW and cs.buckets(d.nk) % 4
