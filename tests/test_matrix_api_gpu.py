"""The host path that kmx_select_*, kmx_colsums_*, kmx_diff_*, kmx_dist_*, kmx_pan_*, kmx_colors_*, kmx_gram_* and kmx_assoc_* share
(matrix_host.hpp), where the tools' own suites do not look: a body without rows through both entries, a kept result read after later
calls have reused its scratch, which limit answers a task that breaks two, and the knobs of pan, colors, gram and assoc.  9 columns (a
ragged PA payload byte, fewer columns than lanes), 300 rows (a tile of 256 and a ragged tail, several chunks of 64), a list of 3.
Expectations from tests/*_ref.py.  Run with -m gpu."""
import ctypes as C
import functools
import numpy as np
import pytest

import assoc_ref as ar
import colors_ref as cr
import diff_ref as fr
import dist_ref as dr
import gram_ref as gr
import pan_ref as pr
import select_ref as sr

pytestmark = pytest.mark.gpu
COUNT, PA, BF, BFC = dr.MODE_COUNT, dr.MODE_PA, 2, 3
N, KW, ROWS, COLS, M = 9, 1, 300, (4, 2, 1), 3
GROUP = np.array([0, 1, 2, 0, 1, 0, 1, 2, 0], np.uint8)
T0, T1 = 5003, 6997                                   # the groups' totals over "the whole run"
WEIGHTS = np.array([0, 5, 1, 0xFFFFFFFF], np.uint32)  # M + 1 class weights
VECS = ar.make_vecs("random", M, 2, 77)
DIFF_MIN_REC = 3      # (of 7 control and case columns: some rows of every body fall short)
ASSOC = dict(frac_bits=30, gain=3.7, vmin=2.0 ** -10, threshold=0.0, cols=COLS, min_rec=1)
TOOLS = ["select", "colsums", "diff", "dist", "pan", "colors", "gram", "assoc"]
OK, INVAL, UNSUP = 0, -2, -5


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def body_of(mode, i):
    """three bodies a mode; i = None: no rows"""
    return dr.make_body(500 + 10 * mode + i, ROWS, N, KW, mode, fill=0.5, maxed=0.02) if i is not None else np.zeros(0, np.uint8)


def args_of(tool, mode):
    """what follows (body or pointer, n_rows, N, KW, mode) in the tool's call"""
    return {"select": dict(cols=COLS, min_rec=1), "colsums": {}, "diff": dict(group=GROUP, total_ctrl=T0, total_case=T1, threshold=0.0, min_rec=DIFF_MIN_REC),
            "dist": dict(mins=mode == COUNT), "pan": dict(cols=COLS, shared=True), "colors": dict(cols=COLS), "gram": dict(weights=WEIGHTS, cols=COLS),
            "assoc": dict(vecs=VECS, **ASSOC)}[tool]


def call(ctx, tool, entry, mode, body, keep=False, **more):
    """the tool's call on a body through the host or the device entry -> its output, or with keep the waited-for result"""
    n_rows = len(body) // dr.row_bytes(KW, N, mode)
    kw = {**args_of(tool, mode), **more}
    if entry == "host":
        return getattr(ctx, tool)(body, n_rows, N, KW, mode, keep=keep, **kw)
    import torch
    d = torch.from_numpy(np.ascontiguousarray(body).copy()).to("cuda:0") if n_rows else None
    torch.cuda.synchronize()
    r = getattr(ctx, tool + "_dev")(d.data_ptr() if n_rows else None, n_rows, N, KW, mode, keep=True, **kw)
    try:
        r.wait()      # (the tensor may go once the call has run)
        out = r if keep else r.output()
    except BaseException:
        r.free()
        raise
    if not keep:
        r.free()
    return out


@functools.lru_cache(maxsize=None)
def expected(tool, mode, i):
    b = body_of(mode, i)
    if tool == "select":
        return sr.select_expected_np(b, N, KW, mode, cols=COLS, min_rec=1)
    if tool == "colsums":
        return fr.colsums_np(b, N, KW, mode)
    if tool == "diff":
        return fr.diff_expected_mixed(b, N, KW, mode, GROUP, T0, T1)
    if tool == "dist":
        return dr.dist_expected_np(b, N, KW, mode, mins=mode == COUNT)
    if tool == "pan":
        return pr.pan_expected_np(b, N, KW, mode, cols=COLS)
    if tool == "colors":
        return cr.colors_expected_np(b, N, KW, mode, cols=COLS)
    if tool == "gram":
        return gr.gram_expected_np(b, N, KW, mode, WEIGHTS, cols=COLS)
    return ar.assoc_expected_np(b, N, KW, mode, VECS, 30, 3.7, 2.0 ** -10, 0.0, cols=COLS, min_rec=1)


def same(tool, mode, out, i, what):
    """the tool's output on body i against the model, as the tool's own suite compares them"""
    exp, b = expected(tool, mode, i), body_of(mode, i)
    rb = dr.row_bytes(KW, N, mode)
    if tool == "select":
        assert out.body == exp[0] and out.recs.tobytes() == exp[1].tobytes() and 0 < len(exp[1]) < ROWS, what
    elif tool == "colsums":
        assert out.dtype == np.uint64 and np.array_equal(out, exp), what
    elif tool == "diff":      # threshold 0 keeps every row that meets min_rec: no tolerance band (diff_ref.keep_expected)
        idx = [r for r, x in enumerate(exp) if x["r0"] + x["r1"] >= DIFF_MIN_REC]
        assert out.recs["row"].tolist() == idx and 0 < len(idx) < ROWS, what
        for name, key in (("sum_ctrl", "c0"), ("sum_case", "c1"), ("rec_ctrl", "r0"), ("rec_case", "r1"), ("over", "over")):
            assert out.recs[name].tolist() == [exp[r][key] for r in idx], f"{what}: {name}"
        for q, r in zip(out.recs, idx):
            assert abs(exp[r]["stat"] - float(q["stat"])) <= exp[r]["tol"], f"{what}: the statistic of row {r}"
        assert out.body == np.asarray(b).reshape(-1, rb)[idx].tobytes(), what
    elif tool == "dist":
        assert np.array_equal(out.inter, exp[0]) and (np.array_equal(out.mins, exp[1]) if mode == COUNT else out.mins is None), what
    elif tool == "pan":
        assert out.spectrum.tobytes() == exp[0].tobytes() and out.shared.tobytes() == exp[1].tobytes(), what
    elif tool == "colors":
        assert out.n_classes == exp[0] and all(g.tobytes() == e.tobytes() for g, e in zip((out.ids, out.first, out.sizes, out.patterns), exp[1:])), what
    elif tool == "gram":
        assert out.table.shape == (N, N) and out.table.tobytes() == exp.tobytes(), what
    else:
        recs, kept = exp
        assert out.recs.tobytes() == recs.tobytes() and out.body == kept and 0 < len(recs) < ROWS, what


def algo_bytes_no_rows(tool, mode):
    """the family's formula at n_rows = 0: the tables written"""
    return {"select": 0, "colsums": 8 * N, "diff": 0, "dist": 8 * N * N * (2 if mode == COUNT else 1), "pan": 24 * (M + 1) + 8 * (M + 1) * N, "colors": 0,
            "gram": 8 * N * N, "assoc": 4 * N * 2}[tool]


def tables_of(tool, mode, r):
    """(copy call, entries) of every table a result owns"""
    if tool in ("select", "diff", "assoc"):
        return [("copy_body", r.body_bytes()), ("copy_recs", r.rows())]
    if tool == "colors":
        return [("copy_ids", r._rows), ("copy_first", r.n_classes()), ("copy_sizes", r.n_classes()), ("copy_patterns", r.n_classes())]
    return {"colsums": [("copy_sums", N)], "dist": [("copy_inter", N * N)] + ([("copy_mins", N * N)] if mode == COUNT else []),
            "pan": [("copy_spectrum", 3 * (M + 1)), ("copy_shared", (M + 1) * N)], "gram": [("copy_table", N * N)]}[tool]


def too_small_is_refused(tool, mode, r):
    """every table of the result with an entry to copy: a destination one entry short is KMX_E_INVAL"""
    from kmtricks_amd import lib
    n = 0
    for name, entries in tables_of(tool, mode, r):
        if entries:
            buf = np.zeros(64 * entries, np.uint8)
            assert getattr(lib._lib, f"kmx_{tool}_result_{name}")(r._h, buf.ctypes.data, entries - 1) == INVAL, (tool, name)
            assert lib._lib.kmx_last_error(r._ctx._h).decode() == "destination too small"
            n += 1
    return n


@pytest.mark.parametrize("mode", [COUNT, PA], ids=["count", "pa"])
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("tool", TOOLS)
def test_no_rows(ctx, tool, entry, mode):
    r = call(ctx, tool, entry, mode, body_of(mode, None), keep=True)
    try:
        out = r.output()
        if tool in ("select", "diff", "assoc"):
            assert r.rows() == 0 and r.body_bytes() == 0 and out.body == b"" and len(out.recs) == 0
        elif tool == "colors":
            assert r.n_classes() == 0 and out.n_classes == 0 and not len(out.ids) and not len(out.first) and not len(out.sizes) and out.patterns.shape == (0, 1)
        elif tool == "colsums":
            assert out.shape == (N,) and not out.any()
        elif tool == "dist":
            assert out.inter.shape == (N, N) and not out.inter.any() and (out.mins is None if mode == PA else out.mins.shape == (N, N) and not out.mins.any())
        elif tool == "pan":
            assert out.spectrum.shape == (3, M + 1) and not out.spectrum.any() and out.shared.shape == (M + 1, N) and not out.shared.any()
        else:
            assert out.table.shape == (N, N) and not out.table.any()
        assert r.algo_bytes() == algo_bytes_no_rows(tool, mode)
        # (kept rows, records and classes: no entry, nothing can be too small; test_kept_result_after_later_calls asks with rows)
        assert too_small_is_refused(tool, mode, r) == (0 if tool in ("select", "diff", "assoc", "colors") else len(tables_of(tool, mode, r)))
    finally:
        r.free()


@pytest.mark.parametrize("mode", [COUNT, PA], ids=["count", "pa"])
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("tool", TOOLS)
def test_kept_result_after_later_calls(ctx, tool, entry, mode):
    a = call(ctx, tool, entry, mode, body_of(mode, 0), keep=True)
    try:      # (a result is freed before its context goes, whatever fails here)
        a.wait()
        for i in (1, 2):      # the pool hands A's former scratch out again
            same(tool, mode, call(ctx, tool, entry, mode, body_of(mode, i)), i, f"{tool}: a later call")
        same(tool, mode, a.output(), 0, f"{tool}: the kept result")
        same(tool, mode, a.output(), 0, f"{tool}: the kept result, read again")
        assert too_small_is_refused(tool, mode, a) == len(tables_of(tool, mode, a))
    finally:
        a.free()
    a.free()


# ---- first limit wins: tasks that break two limits of the shared checker; the code and text of the one the family's order puts first ----
BLOOM = {"select": ": a Bloom row's identity is its position", "pan": ": a Bloom row is a hash bit, its recurrence is not a k-mer's",
         "colors": ": a Bloom row is a hash bit, its sample set is not a k-mer's", "gram": ": a Bloom row is a hash bit, its recurrence is not a k-mer's",
         "assoc": ": a Bloom row is a hash bit, its presence pattern is not a k-mer's", "diff": "", "colsums": ""}
NO_COLUMN = ": a matrix has at least one column"
MANY_ROWS = ": more than 2^32 - 256 rows in one call (send the body in runs of rows)"


def broken_tasks(tool):
    """(task fields over the valid ones, code, text behind the entry's name)"""
    if tool == "dist":
        return [(dict(n_cols=0, mode=7), INVAL, NO_COLUMN),
                (dict(mode=BFC, key_words=0), UNSUP, ": counting Bloom filter and transposed bodies are not supported (KMX_MODE_COUNT, KMX_MODE_PA and KMX_MODE_BF only)"),
                (dict(n_rows=5, n_cols=2 ** 30), INVAL, ": null rows")]                      # null rows, and a row of 8 + 2^32 bytes
    bloom = ": Bloom filter bodies are not supported" + BLOOM[tool] + " (KMX_MODE_COUNT and KMX_MODE_PA only)"
    if tool in ("diff", "colsums"):
        return [(dict(mode=BF, key_words=0), UNSUP, bloom), (dict(n_cols=0, mode=7), INVAL, NO_COLUMN),
                (dict(key_words=5, n_rows=2 ** 32), INVAL, ": key_words must be 1 ... 4"),
                (dict(n_cols=2 ** 30, n_rows=2 ** 32), UNSUP, ": rows of 4 GiB and more")]
    n_list = "n_out" if tool == "select" else "n_use"
    pa = dict(mode=PA, out_mode=PA) if tool == "select" else dict(mode=PA)
    return [(dict(mode=BF, key_words=0), UNSUP, bloom),
            (dict(n_cols=0, mode=7), INVAL, NO_COLUMN + ", and so has the " + ("selection" if tool == "select" else "list")),
            (dict(min_abund=2, flags=2, **pa), INVAL, ": min_abund above 1 needs counts"),
            (dict(cols=(4, 2, 4), n_rows=2 ** 32), UNSUP, MANY_ROWS),
            (dict(cols=None, **{n_list: 12}), INVAL, ": more " + ("output" if tool == "select" else "listed") + " columns than input columns"),   # and the identity with M != N
            (dict(key_words=0, min_abund=0), INVAL, ": key_words must be 1 ... 4")]


def task_of(tool, hold, **over):
    """the tool's valid task (no rows) with some fields overwritten; hold keeps its arrays alive"""
    from kmtricks_amd import lib
    cols = over.pop("cols", COLS)
    cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
    hold.append(cc)
    f = dict(key_words=KW, mode=COUNT, n_cols=N, rows=None, n_rows=0)
    if tool == "colsums":
        f.update(reserved=0, sums=None)
    elif tool == "diff":
        f.update(min_rec=0, group=GROUP.ctypes.data, total_ctrl=T0, total_case=T1, threshold=0.0)
    elif tool == "dist":
        f.update(want_mins=0, inter=None, mins=None)
    else:
        f.update(cols=None if cc is None else cc.ctypes.data, min_abund=1, flags=0)
        f.update({"n_out" if tool == "select" else "n_use": N if cc is None else len(cc)})
        if tool == "select":
            f.update(min_rec=0, max_rec=0xFFFFFFFF, out_mode=COUNT, reserved=0)
        elif tool == "pan":
            f.update(spectrum=None, shared=None)
        elif tool == "gram":
            f.update(weights=WEIGHTS.ctypes.data, table=None)
        elif tool == "assoc":
            f.update(vecs=VECS.ctypes.data, n_vec=2, frac_bits=30, gain=3.7, vmin=0.0, threshold=0.0, min_rec=0, max_rec=0xFFFFFFFF)
    f.update(over)
    return getattr(lib, f"Kmx{tool.capitalize()}Task")(**f)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("tool", TOOLS)
def test_first_limit_wins(ctx, tool, entry):
    from kmtricks_amd import lib
    who = f"kmx_{tool}_{entry}"
    fn = getattr(lib._lib, who)
    for over, code, text in broken_tasks(tool):
        hold, res = [], C.c_void_p()
        t = task_of(tool, hold, **over)
        assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (who, over)
        assert lib._lib.kmx_last_error(ctx._h).decode() == who + text, (who, over)
    # the valid task is taken, and the context runs a normal call
    hold, res = [], C.c_void_p()
    t = task_of(tool, hold)
    assert fn(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
    getattr(lib._lib, f"kmx_{tool}_result_free")(res)
    same(tool, COUNT, call(ctx, tool, entry, COUNT, body_of(COUNT, 0)), 0, f"{tool}: after the refusals")


@pytest.mark.parametrize("mode", [COUNT, PA], ids=["count", "pa"])
@pytest.mark.parametrize("tool", ["pan", "colors", "gram", "assoc"])
def test_knobs_still_bite(ctx, tool, mode, monkeypatch):
    """one CU planned for and one workgroup a launch: every stride loop makes all its trips, the result is the same"""
    plain = call(ctx, tool, "host", mode, body_of(mode, 0))
    monkeypatch.setenv(f"KMX_{tool.upper()}_CUS", "1")
    monkeypatch.setenv(f"KMX_{tool.upper()}_GRID", "1")
    forced = call(ctx, tool, "host", mode, body_of(mode, 0))
    same(tool, mode, plain, 0, f"{tool}: no knob")
    same(tool, mode, forced, 0, f"{tool}: one CU, one workgroup")
