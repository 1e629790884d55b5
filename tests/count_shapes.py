"""The launch shapes of kmx_count_reads_dev's sync-free path, restated in plain integers, and seeded inputs that
reach each of them: every grid on that path is computed from the data (reads, bases, partitions, k-mers per partition), so the
inputs ARE the knobs.  tests/test_count_shapes_cpu.py holds the constants below against skf.hpp / count_sort.hpp and checks the
builders; tests/test_count_shapes_gpu.py runs them."""
import ctypes as C
import re

import numpy as np

import orc

# ---- the constants the shapes rest on (skf.hpp, count_sort.hpp, count.hip; test_count_shapes_cpu.py reads them out of the headers) ----
SKF_RPW = 16                       # reads a chunk (a wave of the walk)
SKF_MAXP = 1024                    # partitions the path takes
SKF_DK = 1024                      # k-mers a decode block
WPG_STEPS = ((256, 16), (512, 8), (SKF_MAXP, 4))      # skf_wpg: P <= bound -> chunks (waves) a row
SCAN_MAX_WG = 128                  # k_sk_scan: at most so many workgroups ...
SCAN_MIN_ROWS = 32                 # ... of at least so many rows
CS_TARGET = 416                    # cs_target: k-mers a bucket
CS_MAXB = 2048                     # buckets a partition
CS_WALK_TPB = 1024
CS_WALK = {1: 16, 2: 16}           # CsCap<>::walk by key words: keys a thread of a walk chunk
CS_SAMPLE = {1: 16384, 2: 8192}    # CsCap<>::sample
CS_SCAN_MW = 4096                  # buckets a workgroup of k_cs_scan_mw


def ceil_div(a, b):
    return -(-a // b)


def skf_wpg(P):
    for bound, w in WPG_STEPS:
        if P <= bound:
            return w
    return WPG_STEPS[-1][1]


def cs_chunk(key_words):
    """keys of a walk chunk (a workgroup of k_cs_walk)"""
    return CS_WALK[key_words] * CS_WALK_TPB


def cs_schunk(key_words):
    """keys of a staged chunk (a workgroup of k_cs_scatter_staged: 64 KB of keys)"""
    return 65536 // (8 * key_words)


def plan(reads, bases, P, key_words):
    """what the host plans for a sync-free call (superk.hip, the `fast` block) -> the numbers of the `[kmx count_reads_plan]` trace line
    (+ nd_cap, the records the sorted arrays take).  key_words: 1 (k <= 32, or window hashes) or 2 (k = 33 .. 63)"""
    wpg = skf_wpg(P)
    chunks = ceil_div(reads, SKF_RPW)
    rows = ceil_div(chunks, wpg)
    rpg = max(SCAN_MIN_ROWS, ceil_div(rows, SCAN_MAX_WG))
    pbits = 1
    while (1 << pbits) < P:
        pbits += 1
    tb_max = bases // CS_TARGET + P + 1
    return dict(reads=reads, chunks=chunks, rows=rows, wpg=wpg, Gc=ceil_div(rows, rpg), rpg=rpg, pbits=pbits, tb_max=tb_max,
                nc_max=bases // cs_chunk(key_words) + P + 1, nb_max=ceil_div(bases, SKF_DK) + 1, scan_mw=ceil_div(tb_max + 1, CS_SCAN_MW),
                nd_cap=min(bases, bases // 4 + reads + 1024))


def nb_of(n):
    """buckets of a partition of n k-mers (k_sk_scan: at least one)"""
    return max(1, ceil_div(n, CS_TARGET))


def buckets(nk_per_partition):
    """TB: the real buckets of a call"""
    return sum(nb_of(int(n)) for n in nk_per_partition)


def walk_chunks(nk_per_partition, key_words):
    """NC: the real walk chunks of a call"""
    return sum(ceil_div(int(n), cs_chunk(key_words)) for n in nk_per_partition)


PLAN_KEYS = ("reads", "chunks", "rows", "wpg", "Gc", "rpg", "pbits", "tb_max", "nc_max", "nb_max", "scan_mw")
_PLAN_RE = re.compile(r"\[kmx count_reads_plan\] " + " ".join(rf"{k} (\d+)" for k in PLAN_KEYS))
_FAST_RE = re.compile(r"\[kmx count_reads_fast\] records (\d+) k-mers (\d+) buckets (\d+) walk chunks (\d+) listed buckets (\d+) status (\d+) overflow (\d+); the buckets (by counting first|by the full sort)")
HANDED_BACK = "the sync-free path handed the call back"


def trace_plans(err):
    """the `[kmx count_reads_plan]` lines of a stderr capture -> [dict]"""
    return [dict(zip(PLAN_KEYS, map(int, mt.groups()))) for mt in _PLAN_RE.finditer(err)]


def trace_fast(err):
    """the `[kmx count_reads_fast]` lines -> [dict(records, kmers, TB, NC, listed, status, overflow, road)]"""
    names = ("records", "kmers", "TB", "NC", "listed", "status", "overflow")
    return [dict(zip(names, map(int, mt.groups()[:7])), road=mt.group(8)) for mt in _FAST_RE.finditer(err)]


# ---- inputs: one numpy blob + offsets, as Context.pack_reads gives them ------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _copies(rng, n, share):
    """src[i]: the read that read i repeats (itself: an original; a copy repeats an EARLIER original); read 0 is an original"""
    is_copy = rng.random(n) < share
    is_copy[0] = False
    orig = np.nonzero(~is_copy)[0]
    src = np.arange(n)
    ci = np.nonzero(is_copy)[0]
    src[ci] = orig[(rng.random(len(ci)) * np.searchsorted(orig, ci)).astype(np.int64)]
    return src


def _assemble(rng, lengths, src, n_share=0.0, all_n=()):
    """the reads of `lengths` (originals: random bases; read i with src[i] != i repeats read src[i]) -> (blob bytes, uint64 offsets)"""
    n = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)[src]
    is_orig = src == np.arange(n)
    olen = np.where(is_orig, lengths, 0)
    ostart = np.concatenate(([0], np.cumsum(olen)))
    pool = _ACGT[rng.integers(0, 4, int(ostart[-1]))]
    if n_share > 0:      # an N at a random place of a share of the originals
        hit = np.nonzero(is_orig & (lengths > 0) & (rng.random(n) < n_share))[0]
        pool[ostart[hit] + (rng.random(len(hit)) * lengths[hit]).astype(np.int64)] = ord("N")
    for i in all_n:
        pool[ostart[i]:ostart[i] + olen[i]] = ord("N")
    offs = np.concatenate(([0], np.cumsum(lengths)))
    idx = np.repeat(ostart[src] - offs[:-1], lengths) + np.arange(int(offs[-1]))
    return pool[idx].tobytes(), offs.astype(np.uint64)


def short_reads(n, k, seed=1, n_share=0.04, copy_share=0.3):
    """n reads whose cost is in their number: lengths 0 .. k + 11 (at most 12 k-mers), read 0 of full length, then -- as far as n goes -- an
    empty read, reads of k - 1, k and k + 1 bases and a read of N only; a share with an N somewhere; a share copies of earlier reads"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, k + 12, n)
    special = [k + 11, 0, k - 1, k, k + 1, k + 3]
    lengths[:min(n, 6)] = special[:n]
    src = _copies(rng, n, copy_share)
    src[:min(n, 6)] = np.arange(min(n, 6))
    return _assemble(rng, lengths, src, n_share, all_n=(5,) if n > 5 else ())


def exact_kmers(total, k, seed=1, cmax=120):
    """reads without N whose k-mers sum to `total` exactly (a read of k - 1 + c bases gives c, 1 <= c <= cmax); about half are copies"""
    rng = np.random.default_rng(seed)
    N = total // 20 + 8
    c = rng.integers(1, cmax + 1, N)
    src = _copies(rng, N, 0.5)
    cs = np.cumsum(c[src])
    assert cs[-1] >= total
    cut = int(np.searchsorted(cs, total))      # the first read that brings the sum to `total` or beyond: it takes what is missing
    c, src = c[:cut + 1].copy(), src[:cut + 1].copy()
    src[cut] = cut
    c[cut] = total - (int(cs[cut - 1]) if cut else 0)
    return _assemble(rng, k - 1 + c, src)


def fixed_reads(n, length, seed=1, copy_share=0.25):
    """n reads of `length` bases without N, a share of them copies"""
    rng = np.random.default_rng(seed)
    return _assemble(rng, np.full(n, length), _copies(rng, n, copy_share))


def filled_then_empty(Q, P, m):
    """a repartition table for nb_parts = P > Q that sends every minimizer to partitions 0 .. Q - 1: the P - Q trailing partitions stay empty
    and take exactly one bucket each"""
    assert 0 < Q < P <= SKF_MAXP
    return orc.repart_static(m, Q)


def reads_list(packed):
    blob, offs = packed
    o = offs.astype(np.int64).tolist()
    return [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]


_POOL = {}


def _pool(k, m, seed):
    """a few hundred reads of 0 .. 12 k bases (some with N) and the super-k-mers of each, from the oracle on the single read"""
    if (k, m, seed) not in _POOL:
        rng = np.random.default_rng(seed)
        lengths = np.concatenate((np.arange(0, k + 2), rng.integers(k, 12 * k, 360)))
        reads = reads_list(_assemble(rng, lengths, np.arange(len(lengths)), n_share=0.1))
        lut, one = orc.minimizer_lut(m), np.zeros(4 ** m, dtype=np.uint16)
        counts = np.array([orc.superk_partition([r], k, m, lut, one, 1)[0][2] for r in reads], dtype=np.int64)
        _POOL[(k, m, seed)] = (reads, counts)
    return _POOL[(k, m, seed)]


def chunk_of(descriptors, k=21, m=7, seed=7):
    """16 consecutive reads (one chunk of the walk) whose super-k-mers sum to `descriptors`, picked from a pool: the largest count that still
    fits, slot by slot; then shuffled"""
    reads, counts = _pool(k, m, seed)
    rng = np.random.default_rng(seed + descriptors)
    left, pick = descriptors, []
    for _ in range(SKF_RPW):
        fit = np.nonzero(counts <= left)[0]
        best = fit[counts[fit] == counts[fit].max()]
        i = int(best[int(rng.integers(0, len(best)))])
        pick.append(i)
        left -= int(counts[i])
    assert left == 0, (descriptors, left)
    return [reads[i] for i in rng.permutation(pick)]


# ---- the oracle's answer to a call ---------------------------------------------------------------------------------------------------
def oracle_split(packed, k, m, repart, P):
    """one pass of the oracle over the reads -> ([(record stream, k-mers, super-k-mers)] per partition, pinfo[P, 2 + 1280], super-k-mers per
    minimizer, k-mers per minimizer): what orc.superk_partition and orc.superk_stats give, with one call a read instead of two"""
    lut = orc.minimizer_lut(m)
    repart = np.ascontiguousarray(repart, dtype=np.uint16)
    bufs = (orc.OrcBuf * P)()
    pinfo = np.zeros(P * (2 + 5 * 256), dtype=np.uint64)
    ms, mk, mx = (np.zeros(4 ** m, dtype=np.uint64) for _ in range(3))
    f, args = orc._lib.orc_superk_partition_stats, (k, m, lut.ctypes.data, repart.ctypes.data, P, bufs, pinfo.ctypes.data, ms.ctypes.data, mk.ctypes.data, mx.ctypes.data)
    for s in reads_list(packed):
        rc = f(s, len(s), *args)
        assert rc == 0, rc
    out = []
    for p in range(P):
        out.append((C.string_at(bufs[p].data, bufs[p].len) if bufs[p].len else b"", int(bufs[p].nb_kmers), int(bufs[p].nb_superk)))
        orc._lib.orc_buf_free(C.byref(bufs[p]))
    return out, pinfo.reshape(P, -1), ms, mk


# ---- the shape table: the smallest inputs that reach each edge ------------------------------------------------------------
W_HASH = 1 << 40      # the window of the hashed twins


class Case:
    """id; make() -> (packed reads, k, m, P, repartition table, aim); modes: "plain" | "hashed", "-sort" behind it: the buckets by the full sort
    (KMX_COUNT_HASH_FIRST=0; counting first otherwise, for 64-bit keys); fast: the call stays on the sync-free path (False: it never enters);
    handback: it enters and hands the call back.  aim: numbers of plan() / of the trace (TB, NC) the case is there for."""

    def __init__(self, id, make, modes=("plain", "hashed"), fast=True, handback=False):
        self.id, self.make, self.modes, self.fast, self.handback = id, make, modes, fast, handback


def _split_case(n, P, aim, k=21, m=7, seed=None):
    def make():
        return short_reads(n, k, seed=seed or (1000 + n + P)), k, m, P, orc.repart_static(m, P), aim
    return make


def _fill_case(one_partition):
    """chunks of 16 reads with 0 (a whole row of them: 16 chunks), 1, 63, 64, 65 and 129 descriptors, a partial chunk last; one_partition: every
    minimizer goes to partition 5 of 8, so the chunk of 64 is 64 records of one partition in one step of k_sk_scatter"""
    def make():
        k, m, P = 21, 7, 8
        reads = []
        for d in [0] * 16 + [1, 63, 64, 65, 129, 0, 64, 129]:
            reads += chunk_of(d, k, m)
        reads += chunk_of(65, k, m)[:7]
        offs = np.zeros(len(reads) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
        rep = np.full(4 ** m, 5, dtype=np.uint16) if one_partition else orc.repart_static(m, P)
        return (b"".join(reads), offs), k, m, P, rep, dict(chunks=25, rows=2, wpg=16, Gc=1)
    return make


def _sort_case(total, k, aim):
    def make():
        return exact_kmers(total, k, seed=total % 1000 + k), k, 10, 1, np.zeros(4 ** 10, dtype=np.uint16), dict(aim, kmers=total, wpg=16, pbits=1)
    return make


SCAN_Q, SCAN_K, SCAN_M, SCAN_LEN = 64, 31, 10, 150


def _scan_case(n_reads, tb_aim):
    """tb_aim: the real bucket count, or None: the largest one 1024 partitions give that is no multiple of 4 (it must lie beyond 8192)"""
    def make():
        packed = fixed_reads(n_reads, SCAN_LEN, seed=n_reads)
        filled = oracle_split(packed, SCAN_K, SCAN_M, orc.repart_static(SCAN_M, SCAN_Q), SCAN_Q)[0]
        b = buckets(e[1] for e in filled)
        if tb_aim is None:
            P = SKF_MAXP if (b + SKF_MAXP - SCAN_Q) % 4 else SKF_MAXP - 1
        else:
            P = SCAN_Q + tb_aim - b
        tb = b + P - SCAN_Q
        assert SCAN_Q < P <= SKF_MAXP and (tb_aim is not None or (tb > 2 * CS_SCAN_MW and tb % 4)), (b, P, tb)
        return packed, SCAN_K, SCAN_M, P, filled_then_empty(SCAN_Q, P, SCAN_M), dict(TB=tb, empty_tail=P - SCAN_Q)
    return make


def _cases():
    out = []
    # the split's grids: reads and partitions
    for n, aim in ((1, dict(chunks=1, rows=1)), (15, dict(chunks=1, rows=1)), (16, dict(chunks=1, rows=1)), (17, dict(chunks=2, rows=1)), (65, dict(chunks=5, rows=1)),
                   (240, dict(chunks=15, rows=1)), (257, dict(chunks=17, rows=2))):
        out.append(Case(f"reads-{n}", _split_case(n, 8, dict(aim, wpg=16, Gc=1, pbits=3))))
    for P, wpg, pbits in ((1, 16, 1), (2, 16, 1), (3, 16, 2), (255, 16, 8), (256, 16, 8), (257, 8, 9), (512, 8, 9), (513, 4, 10), (1023, 4, 10), (1024, 4, 10)):
        out.append(Case(f"parts-{P}", _split_case(3000, P, dict(chunks=188, rows=ceil_div(188, wpg), wpg=wpg, pbits=pbits, Gc=1 if wpg > 4 else 2, rpg=32), seed=3000)))      # (47 rows of 4 chunks: two workgroups)
    out.append(Case("parts-1025", _split_case(3000, 1025, dict(), seed=3000), fast=False))
    out.append(Case("chunk-fill", _fill_case(False)))
    out.append(Case("chunk-fill-one-partition", _fill_case(True)))
    out.append(Case("scan-2wg-P1024", _split_case(2049, 1024, dict(chunks=129, rows=33, wpg=4, rpg=32, Gc=2))))
    out.append(Case("scan-2wg-P256", _split_case(8193, 256, dict(chunks=513, rows=33, wpg=16, rpg=32, Gc=2))))
    out.append(Case("scan-3wg-P1024", _split_case(4097, 1024, dict(chunks=257, rows=65, wpg=4, rpg=32, Gc=3))))
    out.append(Case("scan-125wg-P1024", _split_case(262145, 1024, dict(chunks=16385, rows=4097, wpg=4, rpg=33, Gc=125)), modes=("plain",)))
    # the sample sort's layout: one partition, the k-mers to the unit
    both = ("plain", "hashed")
    roads = ("plain", "plain-sort", "hashed", "hashed-sort")
    for kw, k in ((1, 31), (2, 47)):
        sc = cs_schunk(kw)
        for total in (1, 415, 416, 417, 1023, 1024, 1025, sc, sc + 1, 16384, 16385, 425984, 425985, 851968, 851969):
            aim = dict(TB=nb_of(total), NC=ceil_div(total, cs_chunk(kw)))
            modes = ("plain",) if kw == 2 else roads if total in (425984, 425985) else both
            out.append(Case(f"sort-u{64 * kw}-{total}", _sort_case(total, k, aim), modes=modes, handback=total == 851969))
    # the bucket scan across workgroups
    for tb in (4095, 4096, 4097):
        out.append(Case(f"buckets-{tb}", _scan_case(12000, tb), modes=both if tb == 4097 else ("plain",)))
    out.append(Case("buckets-two-carries", _scan_case(26000, None), modes=("plain",)))
    return out


CASES = {c.id: c for c in _cases()}


class Data:
    """a case's input and the oracle's split of it (one pass; shared by the case's modes)"""

    def __init__(self, case):
        self.packed, self.k, self.m, self.P, self.rep, self.aim = case.make()
        self.n_reads, self.bases = len(self.packed[1]) - 1, len(self.packed[0])
        self.exp, self.pinfo, self.ms, self.mk = oracle_split(self.packed, self.k, self.m, self.rep, self.P)
        self.nk = [e[1] for e in self.exp]
        self.nd = sum(e[2] for e in self.exp)

    def key_words(self, mode):
        return 1 if mode.startswith("hashed") else orc.kw_of_k(self.k)

    def plan(self, mode):
        return plan(self.n_reads, self.bases, self.P, self.key_words(mode))


_DATA = [None, None]


def data(case_id):
    """the last case's Data is kept: a case's modes follow each other"""
    if _DATA[0] != case_id:
        _DATA[:] = [case_id, Data(CASES[case_id])]
    return _DATA[1]
