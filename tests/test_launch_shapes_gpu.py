"""The kernels of `kmx diff`, `select`, `filter`, `combine`, `dist` and the four sequence queries at the launch shapes their hosts pick
for matrices far larger than a test can hold.  Two planning knobs of the host code make a small input take
them: KMX_PLAN_CUS, the CU count the heuristics plan for, and KMX_MAX_GRID, the cap on the workgroups of a launch whose kernel strides
over its work.  Every case is compared with the Python restatement of its tool and, byte for byte, with the same call made with the
variable unset: records, bodies, tables and sums are the same bits whatever the shape.  Run with -m gpu."""
import numpy as np
import pytest

import orc
import dist_ref as dr
import diff_ref as fr
import select_ref as sr
import filter_ref as ft
import combine_ref as cr
import query_ref as qr
import kquery_ref as kr
import cquery_ref as cq
import zquery_ref as zr

pytestmark = pytest.mark.gpu
COUNT, PA, BF = dr.MODE_COUNT, dr.MODE_PA, dr.MODE_BF
GRID = 3      # KMX_MAX_GRID of the stride tests


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def both(monkeypatch, name, value, call):
    """call() with both variables unset, then with `name` set -> (the default plan's result, the shaped one's)"""
    for v in ("KMX_PLAN_CUS", "KMX_MAX_GRID"):
        monkeypatch.delenv(v, raising=False)
    plain = call()
    monkeypatch.setenv(name, str(value))
    try:
        shaped = call()
    finally:
        monkeypatch.delenv(name)
    return plain, shaped


def ceil_div(a, b):
    return (a + b - 1) // b


# ---- the chunk of rows of k_diff_score and k_select_score ----------------------------------------------------------------------------
def planned_rw(n_rows, units, cus):
    """rows of a wave's chunk as diff_queue and select_queue plan them (diff.hip, select.hip): rows of 64 units and more take 64, halved
    while the chunks are fewer than 8 waves a SIMD of `cus` CUs, down to 4"""
    rw = 64
    if units >= 64:
        while rw > 4 and n_rows // rw < cus * 4 * 8:
            rw >>= 1
    return rw


def units_of(n_cols, mode):
    return n_cols if mode == COUNT else (n_cols + 7) // 8


SWEEP = [(m, rows) for m in ("count", "pa") for rows in fr.RW_ROWS]


def test_the_sweep_takes_every_chunk_size():
    """a change of the constants cannot quietly collapse the sweep: planned for one CU its row counts give chunks of 4, 8, 16, 32 and
    64 rows, for both modes; planned for the device every one of them gives 4"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for m, N, mode in (("count", 70, COUNT), ("pa", 520, PA)):
        got = [planned_rw(rows, units_of(N, mode), 1) for rows in fr.RW_ROWS]
        print(f"\nRW sweep, {m}: rows {list(fr.RW_ROWS)} -> chunks of {got} rows")
        assert got == [4, 8, 16, 32, 64]
        assert {planned_rw(rows, units_of(N, mode), cus) for rows in fr.RW_ROWS} == {4}
    assert fr.RW_ROWS[-1] % 64 and ceil_div(fr.RW_ROWS[-1], 256) == 9      # a partial last chunk, nine placement tiles


@pytest.mark.parametrize("m,rows", SWEEP)
def test_diff_chunks(ctx, monkeypatch, m, rows):
    """k_diff_score with chunks of 4 ... 64 rows of a wave (`passes = RW`, `u == p`, `lane < RW`), at thresholds 0 and p = 0.05"""
    from test_diff_gpu import compare
    c = fr.case(f"rw-{m}-{rows}")
    assert planned_rw(rows, units_of(c.n_cols, c.mode), 1) == 4 << fr.RW_ROWS.index(rows)
    for thr in c.thresholds:
        call = lambda: ctx.diff(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, c.group, c.totals[0], c.totals[1], thr, c.min_rec)
        plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, call)
        idx = compare(shaped, c, thr, c.min_rec, f"{c.name} thr={thr!r} planned for one CU")
        assert (idx == list(range(rows))) == (thr == 0.0)
        assert shaped.recs.tobytes() == plain.recs.tobytes() and shaped.body == plain.body and shaped.algo_bytes == plain.algo_bytes


SELECT_SWEEP = [("cc", COUNT, COUNT, 70, "perm", 33), ("cp", COUNT, PA, 70, "perm", 33), ("pp", PA, PA, 520, "every-other", 260)]


@pytest.mark.parametrize("rows", fr.RW_ROWS)
@pytest.mark.parametrize("pair,mode,out_mode,N,kind,M", SELECT_SWEEP)
def test_select_chunks(ctx, monkeypatch, pair, mode, out_mode, N, kind, M, rows):
    """k_select_score with chunks of 4 ... 64 rows of a wave, a recurrence range that keeps a proper subset of the rows"""
    from test_select_gpu import same
    i = fr.RW_ROWS.index(rows)
    assert planned_rw(rows, units_of(N, mode), 1) == 4 << i
    kw = 1 + (i + len(pair) + N) % 4
    body = sr.make_body(8100 + 10 * i + N, rows, N, kw, mode, fill=0.5, pad_ones=True, maxed=0.05, lo=1, hi=4)
    cols = sr.make_cols(kind, N, M, 8100 + i)
    a = 2 if mode == COUNT else 1
    rec = sr.select_expected_np(body, N, kw, mode, cols, out_mode=out_mode, min_abund=a)[1]["rec"]
    med = int(np.median(rec))
    for r in (dict(min_rec=med, max_rec=None), dict(min_rec=1, max_rec=med - 1)):
        r.update(out_mode=out_mode, min_abund=a, zero_below=out_mode == COUNT)
        exp = sr.select_expected_np(body, N, kw, mode, cols, **r)
        assert 0.1 <= len(exp[1]) / rows <= 0.9, (r, len(exp[1]))
        plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, lambda: ctx.select(body, rows, N, kw, mode, cols=cols, **r))
        c = type("C", (), dict(n_rows=rows, key_words=kw, n_cols=N, mode=mode))
        same(shaped, exp, c, f"{pair} rows={rows} {r} planned for one CU")
        assert shaped.recs.tobytes() == plain.recs.tobytes() and shaped.body == plain.body and shaped.algo_bytes == plain.algo_bytes


# ---- a second trip round every stride loop: three workgroups a launch -------------------------------------------------------------
def move_rows(irb):
    """rows of a workgroup of k_filter_move (launch_filter_move): about 128 KB of them, a power of two"""
    sr_ = 256
    while sr_ > 1 and sr_ * irb > 131072:
        sr_ >>= 1
    return sr_


def score_workgroups(n_rows, units):
    """workgroups of four waves that k_diff_score / k_select_score have chunks for (the device's plan)"""
    import torch
    rw = planned_rw(n_rows, units, torch.cuda.get_device_properties(0).multi_processor_count)
    return ceil_div(ceil_div(n_rows, rw), 4)


@pytest.mark.parametrize("name", ["shares-count", "shares-pa"])
def test_diff_strides(ctx, monkeypatch, name):
    """k_diff_score, k_filter_move and k_diff_place (its LDS and barriers meet again every trip) at 16 tiles on 3 workgroups"""
    from test_diff_gpu import compare
    c = fr.case(name)
    irb = dr.row_bytes(c.key_words, c.n_cols, c.mode)
    tiles = ceil_div(c.n_rows, 256)
    assert min(tiles, tiles * (256 // move_rows(irb)), score_workgroups(c.n_rows, units_of(c.n_cols, c.mode))) > 2 * GRID
    for thr in c.thresholds:
        call = lambda: ctx.diff(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, c.group, c.totals[0], c.totals[1], thr, c.min_rec)
        plain, shaped = both(monkeypatch, "KMX_MAX_GRID", GRID, call)
        compare(shaped, c, thr, c.min_rec, f"{c.name} thr={thr!r} on {GRID} workgroups")
        assert shaped.recs.tobytes() == plain.recs.tobytes() and shaped.body == plain.body


def select_stride_cases():
    """the two bodies with proper subsets by design, and of every mode pair the (last) body of 4200 rows: 17 tiles, kept whole or not
    at all"""
    long = {(c.mode, c.out_mode): c.name for c in sr.gpu_cases() if c.n_rows == 4200}
    assert len(long) == 3
    return ["cc-subset", "pp-subset"] + sorted(long.values())


@pytest.mark.parametrize("name", select_stride_cases())
def test_select_strides(ctx, monkeypatch, name):
    """k_select_score, the two movers of k_select_move (or k_filter_move) and k_select_place at 4 and 17 tiles on 3 workgroups"""
    from test_select_gpu import same
    c = sr.case(name)
    tiles = ceil_div(c.n_rows, 256)
    assert min(tiles, score_workgroups(c.n_rows, units_of(c.n_cols, c.mode))) > GRID      # (a mover has a workgroup a tile at the least)
    for r, exp in zip(c.runs, c.expected):
        plain, shaped = both(monkeypatch, "KMX_MAX_GRID", GRID, lambda: ctx.select(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, **r))
        same(shaped, exp, c, f"{name} {r} on {GRID} workgroups")
        assert shaped.recs.tobytes() == plain.recs.tobytes() and shaped.body == plain.body
    assert any(len(e[1]) == c.n_rows if c.n_rows == 4200 else 0 < len(e[1]) < c.n_rows for e in c.expected)


@pytest.mark.parametrize("mode", [COUNT, PA])
@pytest.mark.parametrize("n_cols", [9, 1000])
def test_filter_strides(ctx, monkeypatch, n_cols, mode):
    """k_filter_match (its staged span and its barriers, trip after trip), k_filter_move, k_filter_absent_count and _scatter at 12 tiles
    of rows and of key records on 3 workgroups; m, v and k all asked for"""
    kw, n_rows = 1 + n_cols % 2, 3000
    row_keys, payload, key_keys, key_counts = ft.synth_case(300 + n_cols + mode, n_rows, n_cols, kw, mode, 0.5, 1.0, extreme=True)
    irb = 8 * kw + ft.payload_bytes(n_cols, mode)
    tiles = ceil_div(n_rows, 256)
    assert min(tiles, tiles * (256 // move_rows(irb)), ceil_div(len(key_counts), 256)) > 2 * GRID
    em, ev, eak, eac = ft.filter_expected(row_keys, payload, key_keys, key_counts, mode)
    body = ft.matrix_body(row_keys, payload)
    plain, shaped = both(monkeypatch, "KMX_MAX_GRID", GRID, lambda: ctx.filter(body, n_cols, kw, mode, (key_keys, key_counts), "kmv"))
    assert 0 < shaped.rows < n_rows and 0 < len(eac) < len(key_counts)
    assert shaped.body == em and np.array_equal(shaped.vector, ev)
    assert np.array_equal(shaped.absent_keys, eak) and np.array_equal(shaped.absent_counts, eac)
    assert shaped.body == plain.body and shaped.vector.tobytes() == plain.vector.tobytes()
    assert shaped.absent_keys.tobytes() == plain.absent_keys.tobytes() and shaped.absent_counts.tobytes() == plain.absent_counts.tobytes()


def combine_blocks(what, kw, mode):
    if what == "mixed":      # test_combine_gpu.test_count_files_of_every_width_beside_a_wide_matrix
        return cr.synth_case(21 + kw, [3000, 2500, 700, 2800, 3100], [1, 1, 333, 1, 1], kw, cr.MODE_COUNT, share=0.5, count_bytes=[1, 2, 4, 4, 1], extreme=True)
    rng = np.random.default_rng(what)      # test_combine_gpu.test_block_counts at B = what
    cols = [int(c) for c in rng.choice([1, 2, 3, 8, 13], what)]
    return cr.synth_case(what, [int(r) for r in rng.integers(200, 900, what)], cols, 1, mode, share=0.6, extreme=True)


@pytest.mark.parametrize("what,kw,mode", [(B, 1, mode) for B in (5, 64) for mode in (cr.MODE_COUNT, cr.MODE_PA)] + [("mixed", 1, cr.MODE_COUNT), ("mixed", 2, cr.MODE_COUNT)])
def test_combine_strides(ctx, monkeypatch, what, kw, mode):
    """k_combine_keys, k_combine_rank (both passes: its staged keys and spans are rewritten every trip) and k_combine_move on 3
    workgroups, with and without KMX_COMBINE_DROP_LAST"""
    blocks = combine_blocks(what, kw, mode)
    slots = sum(ceil_div(len(b[0]), 256) + 1 for b in blocks)
    orb = 8 * kw + cr.payload_bytes(sum(b[2] for b in blocks), mode)
    run = 256
    while run > 1 and orb * run > 131072:      # launch_combine_move: rows of a workgroup
        run >>= 1
    for drop in (False, True):
        exp, rows = cr.combine_expected(blocks, kw, mode, drop)
        assert min(slots, ceil_div(rows, run)) > GRID
        plain, shaped = both(monkeypatch, "KMX_MAX_GRID", GRID, lambda: ctx.combine([(cr.block_body(b[0], b[1]), b[2], b[3]) for b in blocks], kw, mode, drop))
        assert shaped.rows == rows and shaped.body == exp, f"{what} drop_last={drop} on {GRID} workgroups"
        assert plain.rows == rows and plain.body == shaped.body


DIST_KW = {COUNT: 1, PA: 1, BF: 0}


def dist_same(out, exp, what):
    assert np.array_equal(out.inter, exp[0]), what
    assert (out.mins is None) if exp[1] is None else np.array_equal(out.mins, exp[1]), what


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
def test_dist_slab_strides(ctx, monkeypatch, mode):
    """k_dist_slab at 79 slab words of 64 rows (N = 100: two blocks of samples) on 3 workgroups of four waves"""
    N, rows, kw = 100, 5000, DIST_KW[mode]
    n_tiles = ceil_div(rows, 64) * (ceil_div(N, 64) if mode == COUNT else ceil_div(ceil_div(N, 64), 8))
    assert ceil_div(n_tiles, 4) > 2 * GRID
    body = dr.make_body(40 + mode, rows, N, kw, mode, 0.3, maxed=0.01)
    exp = dr.dist_expected_np(body, N, kw, mode, mins=mode == COUNT)
    plain, shaped = both(monkeypatch, "KMX_MAX_GRID", GRID, lambda: ctx.dist(body, None, N, kw, mode, mins=mode == COUNT))
    dist_same(shaped, exp, f"mode={mode} on {GRID} workgroups")
    dist_same(plain, exp, f"mode={mode}")
    assert exp[0].any()


def dist_runs(units, pairs, cus, run_min, run_max, step):
    """runs a block pair as dist.hip's dist_runs plans them: 8 workgroups a CU over the pairs, no run below run_min units"""
    r = max(1, cus * 8 // pairs)
    r = min(r, ceil_div(units, run_min))
    r = max(r, ceil_div(units, run_max), 1)
    length = ceil_div(ceil_div(units, r), step) * step
    return ceil_div(units, length)


def planned_runs(rows, N, cus):
    """-> (runs of k_dist_pairs, runs of k_dist_mins) a block pair"""
    pairs = ceil_div(N, 64) * (ceil_div(N, 64) + 1) // 2
    return dist_runs(ceil_div(rows, 64), pairs, cus, 64, 1 << 24, 32), dist_runs(rows, pairs, cus, 256, 1 << 40, 32)


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 64 * 64 - 1, 64 * 64, 64 * 64 + 1, 3 * 64 * 64 + 5])
def test_dist_planned_for_one_cu(ctx, monkeypatch, rows, mode):
    """test_dist_gpu.test_rows' row counts planned for one CU: k_dist_mins takes the longest body in 8 runs, not 49, and k_dist_pairs
    the two-block bodies in 2 runs, not 4"""
    import torch
    N, kw = (9 if mode == COUNT else 70), DIST_KW[mode]
    if rows == 3 * 64 * 64 + 5:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert planned_runs(rows, N, 1) == ((4, 8) if mode == COUNT else (2, 2)) and planned_runs(rows, N, cus)[1] > 8      # (256 CUs: 4 and 49)
    body = dr.make_body(rows + mode, rows, N, kw, mode, 0.4, pad_ones=True)
    exp = dr.dist_expected_np(body, N, kw, mode, mins=mode == COUNT)
    plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, lambda: ctx.dist(body, None, N, kw, mode, mins=mode == COUNT))
    dist_same(shaped, exp, f"rows={rows} mode={mode} planned for one CU")
    dist_same(plain, exp, f"rows={rows} mode={mode}")
    assert bool(exp[0].any()) == (rows > 0)


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
def test_dist_in_one_long_run(ctx, monkeypatch, mode):
    """200 samples are ten block pairs, more than the 8 workgroups planned for one CU: every pair gets one run over all 8197 rows
    (129 slab words; five panels of k_dist_pairs, 257 tiles of k_dist_mins) where the device's plan makes 3 and 33"""
    import torch
    N, rows, kw = 200, 2 * 64 * 64 + 5, DIST_KW[mode]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert planned_runs(rows, N, 1) == (1, 1) and min(planned_runs(rows, N, cus)) > 1      # (256 CUs: 3 and 33)
    body = dr.make_body(500 + mode, rows, N, kw, mode, 0.3, pad_ones=True, maxed=0.01)
    exp = dr.dist_expected_np(body, N, kw, mode, mins=mode == COUNT)
    plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, lambda: ctx.dist(body, None, N, kw, mode, mins=mode == COUNT))
    dist_same(shaped, exp, f"N={N} mode={mode} planned for one CU")
    dist_same(plain, exp, f"N={N} mode={mode}")
    assert exp[0].any()


# ---- the gathers of the sequence queries: eight workgroups a launch ------------------------------------------------------------------
K, M, P, W = 31, 10, 4, 4099
NS = (1, 33, 100, 200, 400, 1000, 2500)      # rows of 1, 2, 4, 7, 13, 32 and 79 dwords: lane groups of 1, 2, 4, ... 64 lanes
PER_READ = 150 - K + 1


@pytest.fixture(scope="module")
def reads():
    """2400 reads of 150 bases (360 kbp, 288 000 k-mers), all but 40 of them from a genome of 3000 bases, so that an index over their
    own k-mers has a few thousand rows"""
    rng = np.random.default_rng(1)
    genome = qr.random_reads(7, 1, 3000)[0]
    seqs = [genome[a:a + 150] for a in rng.integers(0, 3000 - 150, 2360)] + qr.random_reads(8, 40, 150)
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order], orc.repart_static(M, P)


def log_lanes(units):
    """log2 of the lanes of a group: the power of two at or above the units of a row a lane can own, 64 at the most"""
    log_l = 0
    while log_l < 6 and (1 << log_l) < units:
        log_l += 1
    return log_l


def trip_records(log_l, run):
    """records that the eight workgroups a CU of a gather take in one trip: four waves of 64 >> log_l groups, `run` records a group"""
    return 8 * 4 * (64 >> log_l) * run


def reads_for(reads, log_l, run, at_least=0):
    """the first reads of the set whose k-mers make two trips and a half (all 2400 where that is more than the set holds: 288 000
    records, more than the 262 144 of one trip of single lanes at 128 records an item); the count is asserted here"""
    seqs, rep = reads
    n = min(len(seqs), ceil_div(max(5 * trip_records(log_l, run), 2 * at_least), 2 * PER_READ) + 1)
    records = n * PER_READ
    assert records > trip_records(log_l, run), (n, records, log_l, run)
    return seqs[:n], rep, records


def in_chunks(seqs, fn):
    """fn over 100 reads at a time (the numpy roads unpack a positions x N table), the tables put together"""
    parts = [fn(seqs[i:i + 100]) for i in range(0, len(seqs), 100)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(len(parts[0])))


def test_the_gather_cases_take_every_lane_group():
    assert [log_lanes(ceil_div(ceil_div(N, 8), 4)) for N in NS] == [0, 1, 2, 3, 4, 5, 6]                 # query, kquery PA, zquery
    assert sorted({log_lanes(ceil_div(N, 8)) for N in NS + CQ_MORE}) == [0, 1, 2, 3, 4, 5, 6]            # cquery: blocks of 8 columns
    assert sorted({log_lanes(N) for N in NS + KQ_MORE}) == [0, 1, 2, 3, 4, 5, 6]                         # kquery COUNT: columns
    assert trip_records(0, 63) == 129024 and trip_records(0, 128) == 262144 < 2400 * PER_READ


@pytest.mark.parametrize("N", NS)
def test_query_gather(ctx, monkeypatch, reads, N):
    """k_query_gather<LOG_L, false> on 8 workgroups: items of 63 records"""
    seqs, rep, records = reads_for(reads, log_lanes(ceil_div(ceil_div(N, 8), 4)), 63)
    mats, _ = qr.synth_index(100 + N, N, W, P, K, M, 0.3 if N <= 100 else 0.05, pad_ones=True)
    en, eh = in_chunks(seqs, lambda s: zr.zquery_expected_np(s, K, 0, M, rep, W, N, mats))
    assert int(en.sum()) == records and eh.any()
    plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, lambda: ctx.query(seqs, K, M, rep, W, N, mats))
    assert np.array_equal(shaped.n_kmers, en) and np.array_equal(shaped.hits, eh), f"N={N} planned for one CU"
    assert shaped.n_kmers.tobytes() == plain.n_kmers.tobytes() and shaped.hits.tobytes() == plain.hits.tobytes()


@pytest.mark.parametrize("z", [0, 3])
@pytest.mark.parametrize("N", NS)
def test_zquery_rows_and_window(ctx, monkeypatch, reads, N, z):
    """k_zquery_rows (items of 64 records) and k_zquery_window (items of 63 positions) on 8 workgroups"""
    seqs, rep, records = reads_for(reads, log_lanes(ceil_div(ceil_div(N, 8), 4)), 64)
    mats, _ = qr.synth_index(200 + N, N, W, P, K, M, 0.6, pad_ones=True)
    en, eh = in_chunks(seqs, lambda s: zr.zquery_expected_np(s, K, z, M, rep, W, N, mats))
    assert int(en.sum()) == records - z * len(seqs) and eh.any()
    plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, lambda: ctx.zquery(seqs, K, M, rep, W, N, mats, z))
    assert np.array_equal(shaped.n_kmers, en) and np.array_equal(shaped.hits, eh), f"N={N} z={z} planned for one CU"
    assert shaped.n_kmers.tobytes() == plain.n_kmers.tobytes() and shaped.hits.tobytes() == plain.hits.tobytes()


CQ_MORE = (12, 29)      # 2 and 4 blocks of 8 columns: the lane groups of k_cquery_gather that NS leaves out


@pytest.mark.parametrize("N", NS + CQ_MORE)
def test_cquery_gather(ctx, monkeypatch, reads, N):
    """k_cquery_gather on 8 workgroups: items of 128 records, a lane a block of 8 columns"""
    w = {1: 2, 12: 8, 29: 1, 33: 5, 100: 3, 200: 7, 400: 4, 1000: 3, 2500: 2}[N]      # (rows of 1 ... 625 bytes)
    seqs, rep, records = reads_for(reads, log_lanes(ceil_div(N, 8)), 128)
    mats, _ = cq.synth_index_bfc(300 + N, N, W, P, K, M, w, pad_ones=True)
    mc = min(2, (1 << w) - 1)
    exp = cq.np_expected_at(cq.np_addresses(seqs, K, M, rep, W, P), W, N, mats, w, mc)
    assert int(exp[0].sum()) == records and exp[1].any() and exp[2].any()
    plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, lambda: ctx.cquery(seqs, K, M, rep, W, N, mats, w, min_class=mc))
    for got, want in zip((shaped.n_kmers, shaped.hits, shaped.sums), exp):
        assert np.array_equal(got, want), f"N={N} w={w} planned for one CU"
    assert shaped.n_kmers.tobytes() == plain.n_kmers.tobytes() and shaped.hits.tobytes() == plain.hits.tobytes() and shaped.sums.tobytes() == plain.sums.tobytes()


KQ_MORE = (2, 3, 7, 13, 29)      # the lane groups of k_kquery_gather (a lane a column) that NS leaves out


@pytest.mark.parametrize("mode,N", [(PA, N) for N in NS] + [(COUNT, N) for N in NS + KQ_MORE])
def test_kquery_search_and_gather(ctx, monkeypatch, reads, mode, N):
    """k_kquery_search on 32 workgroups, then k_query_gather<LOG_L, true> (PA rows) or k_kquery_gather (count rows: items of 128
    records) on 8; the index holds a share of the reads' own k-mers and near misses of them, at most 8 MB of rows"""
    log_l, run = (log_lanes(ceil_div(ceil_div(N, 8), 4)), 63) if mode == PA else (log_lanes(N), 128)
    seqs, rep, records = reads_for(reads, log_l, run, at_least=3 * 32 * 256)
    assert records > 2 * 32 * 256      # (k_kquery_search: 32 workgroups, a record a thread)
    keys = kr.read_keys(seqs, K, M, rep, P)
    frac = min(0.7, 8e6 / (sum(len(x) for x in keys) * kr.stride_of(K, N, mode)))
    mats, _ = kr.synth_kindex(400 + N, N, P, K, M, mode, seqs, frac, pad_ones=True, zeros=0.2, maxed=0.02, fill=0.3, keys=keys)
    assert sum(len(mt) for mt in mats) <= 8.5e6
    exp = kr.kquery_expected_bulk(seqs, K, M, rep, N, mode, mats)
    assert int(exp[0].sum()) == records and exp[1].any() and (mode == PA or int(exp[2].max()) >= 0xFFFFFFFF)
    call = lambda: ctx.kquery(seqs, K, M, rep, N, 1, mode, mats, sums=mode == COUNT)
    plain, shaped = both(monkeypatch, "KMX_PLAN_CUS", 1, call)
    assert np.array_equal(shaped.n_kmers, exp[0]) and np.array_equal(shaped.hits, exp[1]), f"mode={mode} N={N} planned for one CU"
    assert shaped.n_kmers.tobytes() == plain.n_kmers.tobytes() and shaped.hits.tobytes() == plain.hits.tobytes()
    if mode == COUNT:
        assert np.array_equal(shaped.sums, exp[2]) and shaped.sums.tobytes() == plain.sums.tobytes()
