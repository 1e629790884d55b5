"""The Bloom merge kernels -- k_merge_bf<0/1> (hash:bf:bin, hash:bfc:bin) and k_merge_bft (hash:bft:bin) -- at the shapes a run reaches
and test_merge_gpu.py does not: every lane grouping of k_merge_bf and its step from one pass to several, every bfc field width a
query reads, rows up to the widest one LDS tile takes (and the refusal behind it), windows that end inside a dword, lists that are
clustered, that live at one end of the window or that sit on every tile boundary, and batches of unlike tasks.

Every case is compared with the CPU oracle byte for byte (body, rows, the 6 x N statistics) and, up to 200 k records, with
tests/bloom_ref.py, which test_bloom_ref_cpu.py checks the oracle against.  libkmx prints the tile and range policy of every Bloom task
under KMX_TRACE: the tests assert from that line that they ran the shape they aim at.  Needs an MI355X: run with -m gpu."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest

import orc
from bloom_ref import bloom_expected, layout, cohort, arrays, soft_mins

pytestmark = pytest.mark.gpu

PAIRS = [(1, 0), (0, 0), (2, 0), (2, 2), (1, 1), (3, 1)]      # (recurrence-min, share-min)
TRACE = re.compile(r"\[kmx merge\] bloom task (\d+): (\d+) lists, (\d+) bytes a row, (\d+) rows a tile, (\d+) tiles, (\d+) ranges(?:, (single walk|two walks|no recurrences))?")
KERNEL = {orc.MODE_BF: "k_merge_bf", orc.MODE_BFC: "k_merge_bf", orc.MODE_BFT: "k_merge_bft"}


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def trace(monkeypatch):
    monkeypatch.setenv("KMX_TRACE", "1")
    monkeypatch.delenv("KMX_BFT_TWO_WALKS", raising=False)


def row_bytes_of(mode, n, bitw):
    return (n * bitw + 7) // 8 if mode == orc.MODE_BFC else (n + 7) // 8


def tile_rows(mode, n, bitw=2):
    """rows of a k_merge_bf tile as kmx_merge_dev chooses them: 40 KB of rows, a multiple of 64, at least 64"""
    return max(64, (40960 // row_bytes_of(mode, n, bitw)) & ~63)


class Line(tuple):
    """a task's trace line: (lists, bytes a row, rows a tile, tiles, ranges); .walk: how k_merge_bft met the recurrences"""
    walk = None


class Task:
    def __init__(self, lists, r, s, mode, lower, W, bitw=2, soft=None):
        self.lists, self.r, self.s, self.mode, self.lower, self.W, self.bitw = lists, r, s, mode, lower, W, bitw
        self.soft = soft if soft is not None else soft_mins(len(lists))
        self.arr = arrays(lists)
        self.n_recs = sum(len(c) for _, c in self.arr)
        self._exp = {}

    def with_mins(self, r, s):
        """the same lists under other thresholds (the record arrays are shared)"""
        t = Task.__new__(Task)
        t.__dict__.update(self.__dict__)
        t.r, t.s, t._exp = r, s, {}
        return t

    def expected(self):
        if "orc" not in self._exp:
            self._exp["orc"] = orc.merge_matrix(self.arr, 1, self.soft, self.r, self.s, self.mode, self.lower, self.lower + self.W - 1, self.bitw)
        return self._exp["orc"]


def launch(ctx, tasks):
    """one kmx_merge_host batch (host record pointers into one array) -> a function that runs it: (kernel, [(rows, body, stats)])"""
    from kmtricks_amd import lib
    recs = [lib.pack_records(k, c, 1) for t in tasks for k, c in t.arr]
    blob = np.concatenate(recs + [np.zeros((1, 3), np.uint32)])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    prep, j = [], 0
    for t in tasks:
        n = len(t.arr)
        prep.append(dict(lists=[(blob.ctypes.data + 12 * int(offs[j + i]), int(offs[j + i + 1] - offs[j + i])) for i in range(n)], key_words=1, soft_min=t.soft,
                         rec_min=t.r, share_min=t.s, mode=t.mode, lower=t.lower, upper=t.lower + t.W - 1, bitw=t.bitw))
        j += n
    prep = ctx.prepare(prep)

    def go():
        res = ctx.merge_host(prep)
        try:      # (freed before any assertion can fail: a result must not outlive its context in a failed test's traceback)
            res.wait()
            return res.kernel(), [(res.rows(i), res.body(i), res.stats(i)) for i in range(len(tasks))], blob
        finally:
            res.free()
    return go


def compare(tasks, kernel, got):
    """every task against the oracle, and against the second restatement up to 200 k records"""
    assert kernel == KERNEL[tasks[0].mode]
    for i, t in enumerate(tasks):
        eb, er, es = t.expected()
        rows, body, st = got[i]
        assert rows == er and len(body) == len(eb), (i, rows, er)
        if body != eb:
            bad = np.nonzero(np.frombuffer(body, np.uint8) != np.frombuffer(eb, np.uint8))[0]
            raise AssertionError(f"task {i}: body differs at {len(bad)} bytes, first at {bad[:8]} (a row is {row_bytes_of(t.mode, len(t.lists), t.bitw)} bytes)")
        assert np.array_equal(st, es), (i, st, es)
        if t.n_recs <= 200000:
            pb, pr, ps = bloom_expected(t.lists, t.soft, t.r, t.s, t.mode, t.lower, t.lower + t.W - 1, t.bitw)
            assert (pr, ps) == (er, es.tolist()) and pb == eb, i


def run(ctx, capfd, tasks, twice=False):
    """launch + compare, once or twice.  -> the batch's trace lines [Line] by task"""
    tasks = tasks if isinstance(tasks, list) else [tasks]
    go = launch(ctx, tasks)
    for _ in range(2 if twice else 1):
        capfd.readouterr()
        kernel, got, _ = go()
        err = capfd.readouterr().err
        lines = {}
        for m in TRACE.finditer(err):
            lines[int(m[1])] = Line(int(x) for x in m.groups()[1:6])
            lines[int(m[1])].walk = m[7]
        assert sorted(lines) == list(range(len(tasks))), err[-2000:]
        compare(tasks, kernel, got)
        for i, t in enumerate(tasks):
            assert lines[i][0] == len(t.lists) and lines[i][1] == (row_bytes_of(t.mode, len(t.lists), t.bitw))
    return [lines[i] for i in range(len(tasks))]


# ---------------------------------------------------------------------------------------------------------------- sample counts
@pytest.mark.parametrize("mode,bitw", [(orc.MODE_BF, 2), (orc.MODE_BFC, 3)])
@pytest.mark.parametrize("n", [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 512, 513, 1024, 1025])
def test_bf_sample_counts(ctx, capfd, n, mode, bitw):
    """k_merge_bf gives a list g = 64, 32, ... 1 lanes (the largest power of two with g x N <= 512) and walks the lists in one pass up
    to 512 of them -- base, end and soft-min of a lane's list in registers -- and in several passes beyond, re-reading them per tile:
    both sides of every step, two full tiles and a last one of 37 rows"""
    rt = tile_rows(mode, n, bitw)
    W = 2 * rt + 37
    lists = cohort(31 * n + mode, n, 0, W, 0.2)
    base = Task(lists, 1, 0, mode, 0, W, bitw)
    for k, (r, s) in enumerate(PAIRS):
        t = base.with_mins(r, s)
        if k & 1:      # (the window at 3 W)
            t = Task([{h + 3 * W: c for h, c in l.items()} for l in lists], r, s, mode, 3 * W, W, bitw)
        (_, _, got_rt, tiles, _), = run(ctx, capfd, t)
        assert (got_rt, tiles) == (rt, 3)
        eb, _, es = t.expected()
        if (r, s) == (3, 1) and n >= 3:
            assert any(eb)
        if s > 0 and n >= 2:
            assert int(es[1].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- field widths
def bfc_field(body, rb, row, i, w):
    return (int.from_bytes(body[row * rb:(row + 1) * rb], "big") >> (8 * rb - (i + 1) * w)) & ((1 << w) - 1)


@pytest.mark.parametrize("bitw", [1, 2, 3, 4, 5, 6, 7, 8, 13, 16, 17, 31, 32])
@pytest.mark.parametrize("n", [3, 13, 64, 77])
def test_bfc_field_widths(ctx, capfd, n, bitw):
    """fields that straddle bytes and dwords of the LDS image, counts at which to_n_b changes (every power of two) and caps (2^w - 1:
    from 2^15 at w = 4, from 2^31 at w = 5).  Rows 1 and 2 hold 2^31 and 2^15 in every list: kept under both pairs"""
    W = 200
    for lower in (0, 3 * W):
        lists = cohort(7 * n + bitw, n, lower, W, 0.3, extreme=True)
        for l in lists:
            l[lower + 1], l[lower + 2] = 1 << 31, 1 << 15
        for r, s in [(1, 0), (2, 1)]:
            t = Task(lists, r, s, orc.MODE_BFC, lower, W, bitw)
            run(ctx, capfd, t)
            eb = t.expected()[0]
            rb, cap = row_bytes_of(orc.MODE_BFC, n, bitw), (1 << bitw) - 1
            assert bfc_field(eb, rb, 1, 0, bitw) == min(32, cap) and bfc_field(eb, rb, 2, n - 1, bitw) == min(16, cap)


# ---------------------------------------------------------------------------------------------------------------- windows
WINDOWS = ["1", "7", "8", "63", "64", "65", "rt-1", "rt", "rt+1", "2rt+3"]


@pytest.mark.parametrize("wk", WINDOWS)
@pytest.mark.parametrize("mode,bitw", [(orc.MODE_BF, 2), (orc.MODE_BFC, 3)])
@pytest.mark.parametrize("n", [3, 9, 100])
def test_bf_windows(ctx, capfd, n, mode, bitw, wk):
    """windows that are no multiple of 64, of 8, of 4 bytes: the last tile's dword tail and byte tail with real rows in them (rows of
    1, 2 and 13 bytes for hash:bf:bin; 2, 4 and 38 for bfc), one tile and three.  (The store loop's dword HEAD never runs, here or in
    a batch: a tile starts a multiple of 64 rows into a body that has an allocation of its own, so it starts on a 16-byte boundary)"""
    rt = tile_rows(mode, n, bitw)
    W = {"rt-1": rt - 1, "rt": rt, "rt+1": rt + 1, "2rt+3": 2 * rt + 3}.get(wk) or int(wk)
    for lower, (r, s) in ((0, (1, 0)), (3 * W, (2, 1))):
        lists = cohort(n + W, n, lower, W, 0.2)
        lists[0][lower + W - 1] = 5      # (the last row is never empty)
        (_, _, got_rt, tiles, _), = run(ctx, capfd, Task(lists, r, s, mode, lower, W, bitw))
        assert (got_rt, tiles) == (rt, (W + rt - 1) // rt)


@pytest.mark.parametrize("mode,bitw", [(orc.MODE_BF, 2), (orc.MODE_BFC, 3), (orc.MODE_BFT, 2)])
def test_empty_lists_and_a_single_record_at_upper(ctx, capfd, mode, bitw):
    n, W = 9, 2 * tile_rows(mode, 9, bitw) + 3
    for lower in (0, 3 * W):
        run(ctx, capfd, Task([{} for _ in range(n)], 1, 0, mode, lower, W, bitw))
        one = [{} for _ in range(n)]
        one[n - 1][lower + W - 1] = 7
        t = Task(one, 1, 0, mode, lower, W, bitw)
        run(ctx, capfd, t)
        eb = t.expected()[0]
        if mode == orc.MODE_BFT:      # (sample 8's row: the window's last bit)
            w8 = (W + 7) // 8
            assert eb[8 * w8 + (W - 1) // 8] == 1 << ((W - 1) & 7) and sum(eb) == eb[8 * w8 + (W - 1) // 8]
        else:
            assert any(eb[-row_bytes_of(mode, n, bitw):]) and not any(eb[:-row_bytes_of(mode, n, bitw)])


# ---------------------------------------------------------------------------------------------------------------- widest rows
@pytest.mark.parametrize("mode,n,bitw", [(orc.MODE_BF, 5121, 2), (orc.MODE_BF, 12288, 2), (orc.MODE_BFC, 384, 32)])
def test_bf_widest_rows(ctx, capfd, mode, n, bitw):
    """rows of 641 to 1536 bytes: tiles of 64 rows whatever the row, up to 96 KB of image and 48 KB of cursors in LDS"""
    W = 128
    assert tile_rows(mode, n, bitw) == 64 and row_bytes_of(mode, n, bitw) in (641, 1536)
    for lower, (r, s) in ((0, (1, 0)), (3 * W, (2, 1))):
        t = Task(cohort(n, n, lower, W, 0.24), r, s, mode, lower, W, bitw)
        (_, _, got_rt, tiles, _), = run(ctx, capfd, t)
        assert (got_rt, tiles) == (64, 2) and any(t.expected()[0])


@pytest.mark.parametrize("mode,n,bitw", [(orc.MODE_BF, 12289, 2), (orc.MODE_BFC, 385, 32)])
def test_bf_rows_one_byte_too_wide_are_refused(ctx, capfd, mode, n, bitw):
    from kmtricks_amd import lib
    with pytest.raises(lib.KmxError, match="too wide"):
        ctx.merge_host([dict(lists=[(None, 0)] * n, key_words=1, soft_min=[1] * n, rec_min=1, share_min=0, mode=mode, lower=0, upper=127, bitw=bitw)])
    t = Task(cohort(5, 9, 0, 200, 0.3), 2, 1, mode, 0, 200, bitw)      # (the context is still usable)
    run(ctx, capfd, t)
    assert any(t.expected()[0])


# ---------------------------------------------------------------------------------------------------------------- layouts across ranges
@pytest.mark.parametrize("kind", ["uniform", "clustered", "ends", "edges"])
@pytest.mark.parametrize("mode,bitw,W", [(orc.MODE_BF, 2, 12 * 5120 + 37), (orc.MODE_BFC, 2, 12 * 2560 + 37)])
def test_bf_layouts_across_ranges(ctx, capfd, mode, bitw, W, kind):
    """a task cut into several ranges (32768 records and more per range): k_range_bounds_bf's interpolation search -- it expects
    uniform hashes -- on lists that are clustered, that lie at one end of the window (ranges they never enter), and that hold a record
    on both sides of every tile boundary and on it (the hash a range starts at)"""
    n, lower = 64, 3 * W
    base = Task(layout(kind, 5 + n, n, lower, W, 2200, 64), 1, 0, mode, lower, W, bitw)
    for r, s in [(1, 0), (2, 1), (3, 2)]:
        t = base.with_mins(r, s)
        (_, _, got_rt, tiles, c), = run(ctx, capfd, t)
        assert got_rt == tile_rows(mode, n, bitw) and tiles == 13
        assert c >= 2      # (what the test is about: a device with so many CUs that a range falls below 16384 records needs longer lists here)
        assert any(t.expected()[0]) and (s == 0 or int(t.expected()[2][1].sum()) > 0)


# ---------------------------------------------------------------------------------------------------------------- k_merge_bft
@pytest.mark.parametrize("n", [1, 7, 8, 9, 47, 48, 49, 95, 96, 97, 145, 3841])
def test_bft_sample_counts(ctx, capfd, n):
    """blocks of 48 samples and rows of 8: either side of one, two and three blocks; 3841 samples: the second trip of the prologue's
    search loop (5 x 768 searches per trip)"""
    W = 2048 + 100
    bases = [Task(cohort(n, n, lower, W, 10 / W if n > 1000 else 0.1), 1, 0, orc.MODE_BFT, lower, W) for lower in (0, 3 * W)]
    for k, (r, s) in enumerate(PAIRS):
        t = bases[k & 1].with_mins(r, s)
        (_, rb, _, tiles, _), = run(ctx, capfd, t)
        assert tiles >= 2 and t.expected()[1] == (n + 7) // 8 * 8
        if (r, s) == (3, 1) and n >= 4:
            assert any(t.expected()[0])
        if s > 0 and n >= 2:
            assert int(t.expected()[2][1].sum()) > 0


@pytest.mark.parametrize("W", [8, 64, 72, 128, 1000, 1024, 1025, 2048 + 128])
def test_bft_windows(ctx, capfd, W):
    """the three ways out of a tile: 16-byte stores (a sample's row, the tile's place in it and its bytes all multiples of 16: 128, 1024,
    2176), 8-byte stores (ceil8(W) a multiple of 64: 64), bytes (8, 72, 1000, 1025)"""
    n = 50
    for lower, (r, s) in ((0, (1, 0)), (3 * W, (1, 1)), (0, (2, 1))):
        lists = cohort(W, n, lower, W, 0.2)
        lists[n - 1][lower + W - 1] = 5
        run(ctx, capfd, Task(lists, r, s, orc.MODE_BFT, lower, W))


LAYOUTS = ["uniform", "clustered", "ends", "edges"]
WALKS = {(1, 0): "no recurrences", (2, 1): "two walks", (3, 2): "two walks", (1, 1): "single walk"}


def bft_layout_task(kind):
    n, W = 100, 20 * 1024 + 100
    return Task(layout(kind, 11 + n, n, 3 * W, W, 400, 256), 1, 0, orc.MODE_BFT, 3 * W, W)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_bft_layouts(ctx, capfd, kind):
    """k_merge_bft sizes a sample's first round of a tile from its share of the window (about 20 records here); `ends` and `clustered`
    put a sample's 400 records into one tile of 1024 rows or two: a short first round and several more.  Without recurrences, with
    u16 recurrences (two walks) and with share-min 1 on the single walk, which the trace line names (a process started with
    KMX_BFT_TWO_WALKS set has no single walk: the test fails there)"""
    base = bft_layout_task(kind)
    for (r, s), walk in WALKS.items():
        t = base.with_mins(r, s)
        line, = run(ctx, capfd, t)
        assert line[3] >= 20 and line.walk == walk
        assert any(t.expected()[0]) and (s == 0 or int(t.expected()[2][1].sum()) > 0)


def two_walks_child():
    """(a process of its own, KMX_BFT_TWO_WALKS set before its first hash:bft launch: libkmx reads the variable once per process)
    share-min 1 on one-bit recurrences with two walks, the four layouts, recurrence-min 1 and 0"""
    from kmtricks_amd import lib

    c = lib.Context(0)
    try:
        for kind in LAYOUTS:
            base = bft_layout_task(kind)
            for r in (1, 0):
                t = base.with_mins(r, 1)
                kernel, got, _ = launch(c, [t])()
                compare([t], kernel, got)
                assert any(t.expected()[0]) and int(t.expected()[2][1].sum()) > 0
            print("two walks ok:", kind, flush=True)
    finally:
        c.close()


def test_bft_layouts_two_walks():
    """the two-walk build of the one-bit recurrences on the four layouts, in a child process (see two_walks_child); its trace lines
    say which walk ran"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, KMX_BFT_TWO_WALKS="1", KMX_TRACE="1")
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_merge_bloom_gpu as T; T.two_walks_child()"
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert [l for l in p.stdout.splitlines() if l.startswith("two walks ok")] == [f"two walks ok: {k}" for k in LAYOUTS]
    lines = list(TRACE.finditer(p.stderr))
    assert len(lines) == 2 * len(LAYOUTS) and all(m[7] == "two walks" and int(m[2]) == 100 and int(m[5]) >= 20 for m in lines), p.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------- mixed batches
def test_mixed_batch_bf(ctx, capfd):
    """one launch: 3, 600 and 5121 samples (rows of 1, 75 and 641 bytes; tiles of 40960, 512 and 64 rows; LDS sized for the largest)"""
    tasks = [Task(cohort(1, 3, 0, 1000, 0.2), 1, 0, orc.MODE_BF, 0, 1000),
             Task(cohort(2, 600, 3 * 1029, 1029, 0.1), 2, 2, orc.MODE_BF, 3 * 1029, 1029),
             Task(cohort(3, 5121, 0, 131, 0.2), 1, 1, orc.MODE_BF, 0, 131)]
    lines = run(ctx, capfd, tasks, twice=True)
    assert [l[2] for l in lines] == [40960, 512, 64] and [l[3] for l in lines] == [1, 3, 3]


def test_mixed_batch_bfc(ctx, capfd):
    """field widths 1, 5 and 32 side by side"""
    tasks = [Task(cohort(4, 40, 0, 777, 0.2, extreme=True), 1, 0, orc.MODE_BFC, 0, 777, 1),
             Task(cohort(5, 77, 3 * 1500, 1500, 0.1, extreme=True), 2, 2, orc.MODE_BFC, 3 * 1500, 1500, 5),
             Task(cohort(6, 21, 0, 333, 0.3, extreme=True), 1, 1, orc.MODE_BFC, 0, 333, 32)]
    lines = run(ctx, capfd, tasks, twice=True)
    assert [l[1] for l in lines] == [5, 49, 84]


def test_mixed_batch_bft(ctx, capfd):
    """9, 300 and 49 samples; the second task's recurrence-min 3 takes the whole launch off the one-bit recurrences -- the first and
    the third alone run with them"""
    tasks = [Task(cohort(7, 9, 0, 3000, 0.2), 1, 1, orc.MODE_BFT, 0, 3000),
             Task(cohort(8, 300, 3 * 5001, 5001, 0.05), 3, 0, orc.MODE_BFT, 3 * 5001, 5001),
             Task(cohort(9, 49, 0, 1234, 0.2), 1, 0, orc.MODE_BFT, 0, 1234)]
    run(ctx, capfd, tasks, twice=True)
    run(ctx, capfd, [tasks[0], tasks[2]], twice=True)
    for t in tasks:
        assert any(t.expected()[0])
