"""The host path of kmx_filter_* and kmx_combine_* (matrix_host.hpp), where the tools' own suites do not look: a kept result read after
later calls have taken its scratch from the pool, inputs without rows through both entries, destinations one entry short, and which
limit answers a task that breaks two.  Filter: 9 columns (a ragged PA payload byte, fewer columns than lanes), 300 rows (a tile of 256
and a tail), one-word keys, a key list of 200 records that keeps half of the rows, want = kmv.  Combine: two blocks of 300 and 200 rows
with 9 and 3 columns, share 0.5.  Expectations from tests/filter_ref.py and tests/combine_ref.py.  Run with -m gpu."""
import ctypes as C
import functools
import numpy as np
import pytest

import combine_ref as cr
import filter_ref as fr

pytestmark = pytest.mark.gpu
COUNT, PA, BF, BFC = fr.MODE_COUNT, fr.MODE_PA, 2, 3
N, KW, ROWS, KEYS = 9, 1, 300, 200
B_ROWS, B_COLS = (300, 200), (9, 3)
REC = 8 * KW + 4                        # bytes of a key record
OK, INVAL, UNSUP = 0, -2, -5
TOOLS = ["filter", "combine"]


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case_of(tool, mode, i):
    """three inputs a tool and mode; i = "no rows" / "no key" (filter) and "empty" (combine): the inputs without rows"""
    if tool == "filter":
        seed = 700 + 10 * mode + (i if isinstance(i, int) else 5)
        row_keys, payload, key_keys, key_counts = fr.synth_case(seed, ROWS, N, KW, mode, keep=0.5, key_ratio=0.0 if i == "no key" else KEYS / ROWS)
        if i == "no rows":      # the key list of a whole case, and none of its rows
            row_keys, payload = row_keys[:0], payload[:0]
        assert len(row_keys) == (0 if i == "no rows" else ROWS) and len(key_keys) == (0 if i == "no key" else KEYS)
        return row_keys, payload, key_keys, key_counts
    rows = (0, 0) if i == "empty" else B_ROWS
    blocks = cr.synth_case(800 + 10 * mode + (i if isinstance(i, int) else 5), rows, B_COLS, KW, mode, share=0.5)
    assert [len(b[0]) for b in blocks] == list(rows)
    return blocks


@functools.lru_cache(maxsize=None)
def expected(tool, mode, i):
    c = case_of(tool, mode, i)
    return fr.filter_expected(*c, mode) if tool == "filter" else cr.combine_expected(c, KW, mode)


def out_row_bytes(tool, mode):
    if tool == "filter":
        return 8 * KW + fr.payload_bytes(N, mode) + (4 if mode == COUNT else 0)
    return 8 * KW + cr.payload_bytes(sum(B_COLS), mode)


def call(ctx, tool, entry, mode, i):
    """the tool's call on case i through kmx_<tool>_host or kmx_<tool>_dev -> the waited-for result"""
    from kmtricks_amd import lib
    c = case_of(tool, mode, i)
    if tool == "filter":
        arrays = [np.frombuffer(fr.matrix_body(c[0], c[1]), np.uint8), lib.pack_records(c[2], c[3], KW).view(np.uint8).reshape(-1)]
    else:
        arrays = [np.frombuffer(cr.block_body(b[0], b[1]), np.uint8) for b in c]
    if entry == "dev":
        import torch
        hold = [torch.from_numpy(a.copy()).to("cuda:0") if a.size else None for a in arrays]
        torch.cuda.synchronize()
        ptr = [t.data_ptr() if t is not None else None for t in hold]
    else:
        hold, ptr = arrays, [a.ctypes.data if a.size else None for a in arrays]
    if tool == "filter":
        t = lib.KmxFilterTask(KW, mode, N, lib.filter_want("kmv"), ptr[0], len(c[0]), lib.KmxList(ptr[1], len(c[2])), None, 0)
    else:
        blocks = (lib.KmxBlock * len(c))(*[lib.KmxBlock(p, len(b[0]), b[2], b[3]) for p, b in zip(ptr, c)])
        hold.append(blocks)
        t = lib.KmxCombineTask(KW, mode, len(c), 0, blocks, None)
    res, who = C.c_void_p(), f"kmx_{tool}_{entry}"
    ctx._check(getattr(lib._lib, who)(ctx._h, C.byref(t), C.byref(res)), who)
    r = lib.FilterResult(ctx, res, KW) if tool == "filter" else lib.CombineResult(ctx, res)
    try:
        r.wait()      # (the inputs may go once the call has run)
    except BaseException:
        r.free()
        raise
    return r


def same(tool, mode, r, i, what):
    """the result's output against the model of case i"""
    out, exp = r.output(), expected(tool, mode, i)
    assert out.row_bytes == r.row_bytes() == out_row_bytes(tool, mode), what
    if tool == "filter":
        body, vec, akeys, acounts = exp
        assert out.body == body and out.rows == r.rows() == len(body) // out.row_bytes, what
        assert out.vector.dtype == np.uint32 and np.array_equal(out.vector, vec), what
        assert np.array_equal(out.absent_keys, akeys) and np.array_equal(out.absent_counts, acounts), what
    else:
        assert out.body == exp[0] and out.rows == r.rows() == exp[1], what


def run_and_check(ctx, tool, entry, mode, i, what):
    r = call(ctx, tool, entry, mode, i)
    try:
        same(tool, mode, r, i, what)
    finally:
        r.free()


def tables_of(tool, r):
    """(copy call, entries as the call counts them, bytes of an entry) of every table of a result"""
    from kmtricks_amd import lib
    if tool == "combine":
        return [("copy_body", lib._lib.kmx_combine_result_body_bytes(r._h), 1)]
    return [("copy_body", lib._lib.kmx_filter_result_body_bytes(r._h), 1), ("copy_vector", lib._lib.kmx_filter_result_vector_len(r._h), 4),
            ("copy_absent", lib._lib.kmx_filter_result_absent(r._h) * REC, 1)]


def short_and_null_are_refused(tool, r):
    """every table of the result with something to copy: a destination one entry short and a null destination are KMX_E_INVAL, each
    with its text, and the table is still read whole behind them -> the tables asked"""
    from kmtricks_amd import lib
    n = 0
    for name, entries, size in tables_of(tool, r):
        if entries:
            fn = getattr(lib._lib, f"kmx_{tool}_result_{name}")
            buf = np.zeros(entries * size, np.uint8)
            assert fn(r._h, buf.ctypes.data, entries - 1) == INVAL, (tool, name)
            assert lib._lib.kmx_last_error(r._ctx._h).decode() == "destination too small", (tool, name)
            assert not buf.any(), (tool, name)
            assert fn(r._h, None, entries) == INVAL, (tool, name)
            assert lib._lib.kmx_last_error(r._ctx._h).decode() == "null destination", (tool, name)
            assert fn(r._h, buf.ctypes.data, entries) == OK, (tool, name)
            n += 1
    return n


@pytest.mark.parametrize("mode", [COUNT, PA], ids=["count", "pa"])
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("tool", TOOLS)
def test_kept_result_after_later_calls(ctx, tool, entry, mode):
    a = call(ctx, tool, entry, mode, 0)
    try:      # (a result is freed before its context goes, whatever fails here)
        for i in (1, 2):      # the pool hands A's former scratch out again
            run_and_check(ctx, tool, entry, mode, i, f"{tool}: a later call")
        same(tool, mode, a, 0, f"{tool}: the kept result")
        same(tool, mode, a, 0, f"{tool}: the kept result, read again")
        assert short_and_null_are_refused(tool, a) == len(tables_of(tool, a))
        same(tool, mode, a, 0, f"{tool}: the kept result behind the refusals")
    finally:
        a.free()
    a.free()


NO_ROWS = [("filter", "no rows"), ("filter", "no key"), ("combine", "empty")]


@pytest.mark.parametrize("mode", [COUNT, PA], ids=["count", "pa"])
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("tool,i", NO_ROWS, ids=[f"{t}-{i.replace(' ', '_')}" for t, i in NO_ROWS])
def test_no_rows(ctx, tool, i, entry, mode):
    r = call(ctx, tool, entry, mode, i)
    try:
        same(tool, mode, r, i, f"{tool}, {i}")
        out = r.output()
        assert out.rows == 0 and out.body == b""
        if i == "no rows":      # every record of the key list is absent; kmx.h: the key list read, the absent records written
            assert len(out.vector) == 0 and len(out.absent_counts) == KEYS
            assert r.algo_bytes() == KEYS * REC + KEYS * REC
            assert short_and_null_are_refused(tool, r) == 1
        elif i == "no key":     # the rows' keys read, the vector written
            assert out.vector.shape == (ROWS,) and not out.vector.any() and len(out.absent_counts) == 0 and out.absent_keys.shape == (0, KW)
            assert r.algo_bytes() == ROWS * 8 * KW + 4 * ROWS
            assert short_and_null_are_refused(tool, r) == 1
        else:                   # no input row read, no output row written
            assert r.algo_bytes() == 0
            assert short_and_null_are_refused(tool, r) == 0
    finally:
        r.free()


# ---- first limit wins: tasks that break two limits; the code and the text of the one the tool's order puts first ----
FILTER_BLOOM = ": Bloom filter matrices are not filtered (KMX_MODE_COUNT and KMX_MODE_PA rows of k-mer matrices only; hash matrices neither)"
COMBINE_BLOOM = ": Bloom filter matrices are not combined (KMX_MODE_COUNT and KMX_MODE_PA rows only)"
BROKEN = {
    "filter": [(dict(key_words=5, mode=BF), INVAL, ": key_words must be 1 ... 4"),
               (dict(mode=BFC, n_cols=0), UNSUP, FILTER_BLOOM),
               (dict(mode=7, n_cols=0), INVAL, ": mode must be KMX_MODE_COUNT or KMX_MODE_PA"),
               (dict(n_cols=0, want=0), INVAL, ": a matrix has at least one column"),
               (dict(n_rows=5, rows=None, n_cols=2 ** 30), INVAL, ": null row pointer")],
    "combine": [(dict(key_words=0, mode=BF), INVAL, ": key_words must be 1 ... 4"),
                (dict(mode=BF, flags=2), UNSUP, COMBINE_BLOOM),
                (dict(flags=2, n_blocks=0), INVAL, ": unknown flag (KMX_COMBINE_DROP_LAST is the only one)"),
                (dict(block=dict(n_cols=0, count_bytes=3)), INVAL, ": block 0: a block has at least one column")],
}


def task_of(tool, hold, **over):
    """the tool's valid task (no rows) with some fields overwritten; hold keeps its arrays alive"""
    from kmtricks_amd import lib
    if tool == "filter":
        f = dict(key_words=KW, mode=COUNT, n_cols=N, want=lib.FILTER_M, rows=None, n_rows=0, key=lib.KmxList(None, 0), marks=None, key_on_device=0)
        f.update(over)
        return lib.KmxFilterTask(**f)
    b = dict(rows=None, n_rows=0, n_cols=N, count_bytes=4)
    b.update(over.pop("block", {}))
    blocks = (lib.KmxBlock * 1)(lib.KmxBlock(**b))
    hold.append(blocks)
    f = dict(key_words=KW, mode=COUNT, n_blocks=1, flags=0, blocks=blocks, block_on_device=None)
    f.update(over)
    return lib.KmxCombineTask(**f)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("tool", TOOLS)
def test_first_limit_wins(ctx, tool, entry):
    from kmtricks_amd import lib
    who = f"kmx_{tool}_{entry}"
    fn = getattr(lib._lib, who)
    for over, code, text in BROKEN[tool]:
        hold, res = [], C.c_void_p()
        t = task_of(tool, hold, **over)
        assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (who, over)
        assert lib._lib.kmx_last_error(ctx._h).decode() == who + text, (who, over)
    # the valid task is taken, and the context runs a normal call
    hold, res = [], C.c_void_p()
    t = task_of(tool, hold)
    assert fn(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
    getattr(lib._lib, f"kmx_{tool}_result_free")(res)
    run_and_check(ctx, tool, entry, COUNT, 0, f"{tool}: after the refusals")
