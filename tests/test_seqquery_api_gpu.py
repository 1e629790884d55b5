"""The host path that kmx_query_*, kmx_zquery_*, kmx_kquery_* and kmx_cquery_* share, where the families' own suites do not look:
calls without a query or without a k-mer through both entries, and a kept result read after later calls have reused its scratch.
Expectations from tests/*_ref.py.  Run with -m gpu."""
import numpy as np
import pytest

import cquery_ref as cr
import kquery_ref as kr
import query_ref as qr
import zquery_ref as zr

pytestmark = pytest.mark.gpu
K, M, P, W, N, Z, BITW = 21, 8, 3, 257, 9, 2, 3
FAMILIES = ["query", "zquery", "kquery", "cquery"]


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads():
    """three sets of three reads of at most 100 bases"""
    pool = qr.random_reads(41, 9, 100)
    return [[pool[0], pool[1][:57], pool[2][:K]], [pool[3][:99], pool[4], pool[5][:64]], [pool[6], pool[7][:33], pool[8]]]


class Family:
    """one family: its index over the reads, its host and device call, its expectation as (n_kmers, hits, sums or None)"""

    def __init__(self, name, reads):
        self.name, self.sums = name, name in ("kquery", "cquery")
        if name == "kquery":      # about 200 rows a partition: most of the 9 reads' k-mers
            from kmtricks_amd import lib
            self.mode = lib.MODE_COUNT
            self.mats, self.rep = kr.synth_kindex(5, N, P, K, M, self.mode, [r for rs in reads for r in rs], 0.85, zeros=0.1)
        elif name == "cquery":
            self.mats, self.rep = cr.synth_index_bfc(6, N, W, P, K, M, BITW, pad_ones=True)
        else:
            self.mats, self.rep = qr.synth_index(7, N, W, P, K, M, 0.4, pad_ones=True)

    def host(self, ctx, seqs, mats=None, **kw):
        mats = self.mats if mats is None else mats
        if self.name == "query":
            return ctx.query(seqs, K, M, self.rep, W, N, mats, **kw)
        if self.name == "zquery":
            return ctx.zquery(seqs, K, M, self.rep, W, N, mats, Z, **kw)
        if self.name == "kquery":
            return ctx.kquery(seqs, K, M, self.rep, N, 1, self.mode, mats, **{"sums": True, **kw})
        return ctx.cquery(seqs, K, M, self.rep, W, N, mats, BITW, **kw)

    def dev(self, ctx, seqs, **kw):
        import torch
        from kmtricks_amd import lib
        blob, offs = lib.Context.pack_reads(seqs)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to("cuda:0")
        d_b, d_o, d_r = up(np.frombuffer(blob or b"\0", np.uint8)), up(offs), up(self.rep)
        d_m = [up(mt if len(mt) else np.zeros(1, np.uint8)) for mt in self.mats]
        torch.cuda.synchronize()
        head, rows = (d_b.data_ptr(), d_o.data_ptr(), len(offs) - 1, K, M, d_r.data_ptr()), [t.data_ptr() for t in d_m]
        if self.name == "query":
            return ctx.query_dev(*head, W, N, rows, **kw)
        if self.name == "zquery":
            return ctx.zquery_dev(*head, W, N, rows, Z, **kw)
        if self.name == "kquery":
            n_rows = [len(mt) // kr.stride_of(K, N, self.mode) for mt in self.mats]
            return ctx.kquery_dev(*head, N, 1, self.mode, rows, n_rows, **{"sums": True, **kw})
        return ctx.cquery_dev(*head, W, N, rows, BITW, **kw)

    def expected(self, seqs, mats=None):
        mats = self.mats if mats is None else mats
        if self.name == "query":
            return qr.query_expected(seqs, K, M, self.rep, W, N, mats) + (None,)
        if self.name == "zquery":
            return zr.zquery_expected(seqs, K, Z, M, self.rep, W, N, mats) + (None,)
        if self.name == "kquery":
            return kr.kquery_expected(seqs, K, M, self.rep, N, self.mode, mats)
        return cr.cquery_expected(seqs, K, M, self.rep, W, N, mats, BITW)

    def algo_bytes_no_kmer(self, seqs):
        """the family's formula where no position has a k-mer: the bases read and the tables written"""
        return sum(len(s) for s in seqs) + (12 if self.sums else 4) * len(seqs) * N


@pytest.fixture(scope="module")
def families(reads):
    return {name: Family(name, reads) for name in FAMILIES}


def same(out, exp, what):
    assert np.array_equal(out.n_kmers, exp[0]), f"{what}: n_kmers {out.n_kmers} for {exp[0]}"
    assert np.array_equal(out.hits, exp[1]), f"{what}: hits differ in {np.argwhere(out.hits != exp[1])[:4].tolist()}"
    if exp[2] is not None:
        assert out.sums.dtype == np.uint64 and np.array_equal(out.sums, exp[2]), f"{what}: sums differ in {np.argwhere(out.sums != exp[2])[:4].tolist()}"


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("name", FAMILIES)
def test_no_queries(ctx, families, name, entry):
    f = families[name]
    call = f.host if entry == "host" else f.dev
    out = call(ctx, [])
    assert out.n_kmers.shape == (0,) and out.hits.shape == (0, N) and (not f.sums or out.sums.shape == (0, N))
    short = ["", "ACGTA", "ACGTTGCAACGTTGCAACGT"]      # every read shorter than k
    out = call(ctx, short)
    assert out.n_kmers.shape == (3,) and not out.n_kmers.any() and out.hits.shape == (3, N) and not out.hits.any()
    assert not f.sums or (out.sums.shape == (3, N) and not out.sums.any())
    assert out.algo_bytes == f.algo_bytes_no_kmer(short)


@pytest.mark.parametrize("name", FAMILIES)
def test_kept_result_after_later_calls(ctx, families, reads, name):
    f = families[name]
    exp = [f.expected(rs) for rs in reads]
    assert all(e[0].any() and e[1].any() for e in exp)
    a = f.host(ctx, reads[0], keep=True)
    a.wait()
    for rs, e in zip(reads[1:], exp[1:]):      # the pool hands A's former scratch out again
        same(f.host(ctx, rs), e, f"{name}: a later call")
    same(a.output(), exp[0], f"{name}: the kept result")
    same(a.output(), exp[0], f"{name}: the kept result, read again")
    a.free()
    a.free()


def test_zquery_series(ctx, families, reads):
    from kmtricks_amd import lib
    f, seqs = families["zquery"], reads[0]
    first = f.host(ctx, seqs, [f.mats[0], None, None], last=False, keep=True)      # owns the series' table
    assert first.bits_dev() and not first.hits_dev()
    with pytest.raises(lib.KmxError):
        first.output()
    out = f.host(ctx, seqs, [None, f.mats[1], f.mats[2]], bits_dev=first.bits_dev(), last=True)
    first.free()
    same(out, f.expected(seqs), "zquery: the series")
    same(f.host(ctx, seqs), f.expected(seqs), "zquery: one call")


def test_kquery_without_sums(ctx, families, reads):
    from kmtricks_amd import lib
    f = families["kquery"]
    r = f.host(ctx, reads[0], sums=False, keep=True)
    out = r.output()
    assert out.sums is None
    same(out, f.expected(reads[0])[:2] + (None,), "kquery without sums")
    buf = np.zeros((len(reads[0]), N), np.uint64)
    assert lib._lib.kmx_kquery_result_copy_sums(r._h, buf.ctypes.data, buf.size) == -2      # KMX_E_INVAL
    r.free()
