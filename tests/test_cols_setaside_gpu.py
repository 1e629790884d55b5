"""k_merge_cols' records that are no row keys, set aside once per group of four window slots: the column-blocked pair against
the CPU oracle at the shapes where the lanes' picks, the positions in a wave's slice, the split at the tile's middle row key,
the slice's extension and the counts above 254 that share a group with such records can go wrong.  520 lists (five column
blocks, the last one eight lists wide), tiles of 112 row keys (56 for 128-bit keys).  Needs an MI355X: run with -m gpu.

What the shapes rest on: eight adjacent lanes share a list and a lane has 16 window slots, so a lane's four slots of a group
hold records 8 apart in its list -- a run of 9, 17 or 25 consecutive records that are no row keys puts 2, 3 or 4 marked slots
into one group of some lane.  A wave is eight lists; its slice of half a tile takes 128 entries, the extension 384 more.

Every task has ONE key range, so tile t of a task is row keys 112 t ... 112 t + 111 and its halves split at row key 112 t + 56.
How many ranges a task gets is libkmx's choice (work items wanted / tasks of the batch / column blocks, merge_host.hip): with
KMX_ITEMS_PER_SLOT=1 it wants 256 work items on 256 CUs, and a batch of at least 64 tasks over five (three) column blocks leaves each
task one range -- so every batch here is its sets repeated to 64 tasks or more (the same device lists), as in
test_cols_seeds_gpu.py.  Where the geometry shows from outside it is asserted: 128 entries in one half of a tile complete on the
plain build and 129 do not, 100 in either half of one tile do, 512 fit the EXT build and 513 do not.

The lists are built here key by key: the row keys are the pool keys (nearly every list holds each of them, so the few lists
libkmx merges first -- `witnesses`, the same choice as merge_host.hip's -- agree on them), and everything a case adds goes into
lists that are no witnesses, next to a chosen row key.  No list has keys of its own unless a case gives it some (`sprinkle`:
the everyday records for the slices, in lists that are no witnesses), so the row keys are exactly the pool keys.  (Were libkmx
to choose other lists, the asserts on the kernels' names in the slice tests would fail: they hold only with these tiles.)

Recurrence-min is 1 wherever a case's own keys are held by one list each: every record set aside is then a row of the result,
so an entry that is lost, doubled or put into the other half's slice changes the rows.  (With recurrence-min 2 such a key is
no row and its entry is never seen again; the cases that run with it give their keys to two or more lists.)"""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
N = 520
GAP = 1 << 24          # row keys are at least this far apart: room for a case's own keys next to one
_oracle = {}


def cols_row_lists(rec_min):
    """how many lists the row keys are taken from (merge_host.hip)"""
    for s in range(max(8, rec_min + 2), 33):
        p = 1.0
        for i in range(s - rec_min + 1):
            p *= (s - i) / (i + 1) * 0.035
        if p < 2e-9:
            return s
    return 0


def witnesses(lens, rec_min):
    """the lists libkmx takes the row keys from: the one of median length of each of S stretches of the task"""
    n = len(lens)
    q = min(cols_row_lists(max(1, rec_min)) or 32, n)
    out = []
    for i in range(q):
        w0 = i * n // q
        w1 = max(w0 + 1, (i + 1) * n // q)
        win = sorted(range(w0, w1), key=lambda j: (lens[j], j))
        out.append(win[len(win) // 2])
    return out


def pool_share(pool, n_private, rec_min):
    """the share of the pool a list holds: the largest of 0.97, 0.9, 0.8, 0.7 under which the row keys can be built.  They come from
    a merge of the witnesses in total / 1500 (rounded down, at least one) key ranges, each sorted in LDS, 2048 records at a time: a
    cohort whose ranges would be longer is handed back before the pair starts (8 lists of 0.97 * 300 keys: one range of 2350)."""
    s = cols_row_lists(max(1, rec_min))
    for p in (0.97, 0.9, 0.8, 0.7):
        total = s * (p * pool + n_private)
        if total / max(1, int(total) // 1500) <= 2000:
            return p
    raise AssertionError("no share of the pool fits the row-key merge")


class Case:
    """pool row keys R[0] < R[1] < ...; list i holds each with probability p, plus n_private keys of its own; then the case's
    additions.  Keys are Python ints (64- or 128-bit), turned into arrays by lists()."""

    def __init__(self, seed, pool, kw=1, n=N, rec_min=2, n_private=0, count_lo=2, count_hi=200):
        self.rng = rng = np.random.default_rng(seed)
        p = pool_share(pool, n_private, rec_min)
        self.kw, self.n, self.pool = kw, n, pool
        bits = 61 if kw == 1 else 100
        while True:
            r = sorted({(int(rng.integers(1, 1 << 40)) << (bits - 40)) | int(rng.integers(0, 1 << 20)) for _ in range(pool)})
            if len(r) == pool and all(b - a > 4 * GAP for a, b in zip(r, r[1:])) and r[0] > 4 * GAP:
                break
        self.R = r
        self.recs = []          # per list: {key: count}
        for i in range(n):
            held = rng.random(pool) < p
            cnt = rng.integers(count_lo, count_hi, pool + n_private)
            d = {r[j]: int(cnt[j]) for j in np.flatnonzero(held)}
            for x, (at, o) in enumerate(zip(rng.integers(0, pool, n_private), rng.integers(0, GAP, n_private))):
                d[r[int(at)] + GAP + int(o)] = int(cnt[pool + x])
            self.recs.append(d)
        self.special = set()
        self.sprinkled, self.done = None, False

    def run_after(self, li, row, length, count=3, off=1):
        """`length` consecutive keys R[row] + off ... in list li: records that are no row keys, directly above row key `row`"""
        for x in range(length):
            self.recs[li][self.R[row] + off + x] = count
        self.special.add(li)

    def sprinkle(self, per_list=3, every=4, phase=1):
        """keys of their own for every `every`-th list that the case leaves alone and that is no witness, in place of as many pool
        keys: records for the slices all over the tiles, as any cohort has them.  Done by lists(), behind the case's own changes: the
        lists keep their lengths, so the witnesses stay who they are."""
        self.sprinkled = (per_list, every, phase)
        return self

    def put(self, li, key, count):
        self.recs[li][key] = count
        self.special.add(li)

    def hold_all(self, li, count=5):
        for k in self.R:
            self.recs[li].setdefault(k, count)
        self.special.add(li)

    def lists(self, rec_min):
        lens = [len(d) for d in self.recs]
        w = witnesses(lens, rec_min)
        if self.sprinkled and not self.done:
            per_list, every, phase = self.sprinkled
            for li in range(phase, self.n, every):
                held = [k for k in self.R if k in self.recs[li]]
                if li in w or li in self.special or len(held) < 2 * per_list:
                    continue
                for x in self.rng.choice(len(held), per_list, replace=False):
                    del self.recs[li][held[int(x)]]
                    at = int(self.rng.integers(0, self.pool))
                    self.recs[li][self.R[at] + GAP + int(self.rng.integers(0, GAP))] = int(self.rng.integers(2, 9))
            self.done = True
            assert [len(d) for d in self.recs] == lens
        assert not (set(w) & self.special), "a list the case changed would be one the row keys are taken from"
        assert all(sum(k in self.recs[i] for i in w) >= max(1, rec_min) for k in self.R), "a pool key would be no row key"
        out = []
        for d in self.recs:
            ks = sorted(d)
            k = np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(self.kw)] for v in ks], dtype=np.uint64).reshape(len(ks), self.kw)
            out.append((np.ascontiguousarray(k), np.array([d[v] for v in ks], dtype=np.uint32)))
        return out


@pytest.fixture
def cols(monkeypatch):
    """-> run(sets, kw, soft, rec_min, mode, ...): one batch through the pair, every task against the oracle, `launches` times on
    one context (a slice that overflowed in the first launch makes the second one the EXT build); -> the kernels' names"""
    torch = pytest.importorskip("torch")
    from kmtricks_amd import lib
    monkeypatch.setenv("KMX_MERGE_KERNEL", "cols")
    monkeypatch.setenv("KMX_ITEMS_PER_SLOT", "1")
    made = []

    def run(sets, kw, soft, rec_min, mode, share_min=0, order=True, launches=1, pair=True):
        batch = -(-64 // len(sets))      # 64 tasks or more: one key range a task (see the module's docstring)
        monkeypatch.setenv("KMX_FILE_ORDER", "1" if order else "0")
        ctx = lib.Context(0)
        made.append(ctx)
        ctx.set_file_order(order)
        tasks, exp, keep = [], [], []
        for tag, lists in sets:
            recs = [torch.from_numpy(lib.pack_records(k, c, kw).view(np.int32)).cuda() for k, c in lists]
            keep.append(recs)
            t = dict(lists=[(r.data_ptr(), r.shape[0]) for r in recs], key_words=kw, soft_min=soft, rec_min=rec_min, share_min=share_min, mode=mode)
            tasks += [t] * batch
            key = (tag, kw, rec_min, share_min, mode)
            if key not in _oracle:
                _oracle[key] = orc.merge_matrix([(k.reshape(-1), c) for k, c in lists], kw, soft, rec_min, share_min, mode)
            exp += [_oracle[key]] * batch
        torch.cuda.synchronize()
        kerns = []
        for _ in range(launches):
            res = ctx.merge_dev(tasks)
            res.wait()
            kerns.append(res.kernel())
            for t, (eb, er, es) in enumerate(exp):
                assert res.rows(t) == er, (t, res.rows(t), er)
                assert res.body(t) == eb, f"task {t}: body differs"
                assert np.array_equal(res.stats(t), es), t
            res.free()
        if pair:
            assert all(k == "k_merge_cols" for k in kerns), kerns
        return kerns

    yield run
    for c in made:
        c.close()


SOFT = [1 + (i % 2) for i in range(N)]
RUNS = (1, 9, 17, 25, 40)


def marks_one_list():
    """list 77 holds every row key and runs of 1, 9, 17, 25 and 40 keys between two row keys, in both halves of tiles 0 and 1: 1, 2, 3
    and 4 marked slots in one group of a lane; tile 1 gives it 112 + 17 + 25 + 40 records below its upper key: a second round.  92
    entries in all: no slice overflows, the plain build completes the task"""
    c = Case(11, 460).sprinkle()
    c.hold_all(77)
    for row, n in zip((10, 70, 130, 180, 200), RUNS):
        c.run_after(77, row, n)
    return c


def marks_whole_wave():
    """the eight lists of wave 3 of column block 1 (lists 152 ... 159): each has all five runs, a different length in each of
    five half tiles -- 119 to 174 entries a half tile from the runs alone, beside the other lists' own keys: slices that stay
    below 128 entries and slices that take an extension"""
    c = Case(12, 460).sprinkle(phase=2)
    for j in range(8):
        for h, row in enumerate((10, 70, 130, 180, 240)):
            c.run_after(128 + 24 + j, row, RUNS[(h + j) % 5], off=1 + 100 * j)
    return c


def test_marks_per_lane_and_group(cols):
    cols([("marks-one", marks_one_list().lists(1))], 1, SOFT, 1, orc.MODE_COUNT)


def test_marks_in_every_list_of_a_wave(cols):
    """(the first launch hands the task back for its full slices and is checked like any other; the second is the EXT build)"""
    kerns = cols([("marks-wave", marks_whole_wave().lists(1))], 1, SOFT, 1, orc.MODE_COUNT, launches=2, pair=False)
    assert kerns[1] == "k_merge_cols"


def slice_case(total, half):
    """wave 2 of block 2 (lists 272 ... 279) sets aside exactly `total` records in half `half` of tile 1 (`half` 2: `total` in either
    half), and nobody else has keys of their own"""
    c = Case(1000 + total + 7 * half, 300)
    for h in ((0, 1) if half == 2 else (half,)):
        for j in range(8):
            c.run_after(256 + 16 + j, 112 + 56 * h + 5 + j, total // 8 + (1 if j < total % 8 else 0))
    return c


@pytest.mark.parametrize("half", [0, 1])
def test_slice_just_full_plain_build(cols, half):
    """127 and 128 entries fill a wave's slice of half a tile to the last place but one and to the last: nothing overflows, the plain
    build completes the tasks"""
    cols([(f"slice{t}-{half}", slice_case(t, half).lists(1)) for t in (127, 128)], 1, SOFT, 1, orc.MODE_COUNT)


def test_either_half_has_a_slice_of_its_own(cols):
    """100 entries below and 100 from the middle row key of one tile, one wave: 200 in all, and the plain build completes the task"""
    cols([("slice100-2", slice_case(100, 2).lists(1))], 1, SOFT, 1, orc.MODE_COUNT)


@pytest.mark.parametrize("half", [0, 1])
def test_slice_first_entry_of_the_extension(cols, half):
    """129 in one half of a tile: the plain build hands the tasks back (the first launch, checked like any other), the context's second
    launch is the EXT build, where entry 129 is the first of the extension"""
    kerns = cols([(f"slice129-{half}", slice_case(129, half).lists(1))], 1, SOFT, 1, orc.MODE_COUNT, launches=2, pair=False)
    assert kerns[0] != "k_merge_cols" and kerns[1] == "k_merge_cols", kerns


def test_slice_just_full_ext_build(cols):
    """127, 128 and 129 side by side: the second launch is the EXT build for all of them, and 127 and 128 claim no extension"""
    kerns = cols([(f"slice{t}-1", slice_case(t, 1).lists(1)) for t in (127, 128, 129)], 1, SOFT, 1, orc.MODE_COUNT, launches=2, pair=False)
    assert kerns[1] == "k_merge_cols", kerns


@pytest.mark.parametrize("total", [511, 512])
def test_extension_just_full(cols, total):
    """a slice and its extension take 512 entries: the EXT build completes 511 and 512 (the plain build, first, hands them back)"""
    kerns = cols([(f"slice{total}-0", slice_case(total, 0).lists(1))], 1, SOFT, 1, orc.MODE_COUNT, launches=2, pair=False)
    assert kerns[0] != "k_merge_cols" and kerns[1] == "k_merge_cols", kerns


def test_extension_over(cols):
    """513: handed back by the EXT build too and completed by the next kernel down; equal to the oracle in both launches"""
    kerns = cols([("slice513-0", slice_case(513, 0).lists(1))], 1, SOFT, 1, orc.MODE_COUNT, launches=2, pair=False)
    assert kerns[0] != "k_merge_cols" and kerns[1] != "k_merge_cols", kerns


def middle_case(pool):
    """records that are no row keys directly below and above row key 56 of every tile that has one, below the first row key of the
    range, between the last tile's row keys and above the last row key of all -- in lists of different waves and blocks"""
    c = Case(2000 + pool, pool).sprinkle(phase=3)
    li = [5, 100, 131, 300, 390, 515]
    x = 0
    for t in range((pool + 111) // 112):
        if 112 * t + 56 < pool:
            for d in (-2, -1, 1, 2):
                c.put(li[x % 6], c.R[112 * t + 56] + d, 3 + x); x += 1
        if t:
            for d in (-1, 1):
                c.put(li[x % 6], c.R[112 * t] + d, 3 + x); x += 1      # either side of a tile's first row key
    c.put(li[x % 6], c.R[0] - 5, 7); x += 1
    c.put(li[x % 6], c.R[0] - 4, 7); x += 1
    c.run_after(li[x % 6], pool - 2, 9); x += 1
    c.run_after(li[x % 6], pool - 1, 17)
    return c


@pytest.mark.parametrize("pool", [40, 300, 460])
def test_split_at_the_middle_row_key(cols, pool):
    """pool 40: one tile with fewer than 57 row keys (no second half); 300: the last tile has 76 (a second half of 20); 460: 12"""
    cols([(f"middle{pool}", middle_case(pool).lists(1))], 1, SOFT, 1, orc.MODE_COUNT)


def big_case():
    """row keys with counts of 254, 255, 256 and 70000 in lists 9, 140 and 519, each followed by a run of 9 keys that are no row keys (the
    same lane holds the count and a marked slot, 8 records on), one of them by a run of 25 -- and the same counts on set-aside records"""
    c = Case(31, 460).sprinkle()
    big = (254, 255, 256, 70000)
    for li in (9, 140, 519):
        c.hold_all(li)
        for x, row in enumerate((3, 60, 115, 171, 230, 300, 400, 455)):
            c.recs[li][c.R[row]] = big[x % 4]
            c.recs[li][c.R[row + 1]] = big[(x + 1) % 4]
            c.run_after(li, row, 25 if x == 2 else 9, count=big[(x + 2) % 4] if x % 3 == 0 else 3)
    return c


def test_big_counts_beside_set_aside_records(cols):
    """the NAR build (count rows in file order): a group of four slots with a count for the 4-byte row AND records for the slices"""
    cols([("big", big_case().lists(2))], 1, SOFT, 2, orc.MODE_COUNT)


def recurrence_case(rec_min):
    """keys that are no row keys held by recurrence-min - 1, recurrence-min and recurrence-min + 1 lists of different waves and blocks
    (none of them a list the row keys come from): the first kind is no row, the others are rows k_cols_sparse builds"""
    c = Case(40 + 10 * rec_min, 460, rec_min=rec_min).sprinkle(phase=2)
    holders = [3, 66, 133, 258, 391, 514]
    for x, row in enumerate(range(4, 456, 9)):
        m = rec_min - 1 + x % 3
        for y in range(m):
            c.put(holders[(x + y) % 6], c.R[row] + 1 + x, 2 + (x + y) % 5)
    return c


@pytest.mark.parametrize("rec_min", [1, 2, 3])
def test_recurrence_of_set_aside_keys(cols, rec_min):
    cols([(f"rec{rec_min}", recurrence_case(rec_min).lists(rec_min))], 1, SOFT, rec_min, orc.MODE_COUNT)


def rounds_case(kw=1, n=N):
    """list 200 holds every row key and 60 keys more below tile 1's upper key (172 records: a second round), list 201 has 140 keys
    between two row keys (a round of nothing but such records; its slice overflows: EXT in the second launch); lists 40 ... 47 are
    empty (a whole wave), 230 and 231 are empty too, 48 ... 50 end inside tile 1"""
    c = Case(50 + kw, 300, kw=kw, n=n).sprinkle(phase=3)
    c.hold_all(200)
    c.run_after(200, 150, 60)
    c.run_after(201, 130, 140)
    for li in list(range(40, 48)) + [230, 231]:
        c.recs[li] = {}
    for li in (48, 49, 50):
        c.recs[li] = {k: v for k, v in c.recs[li].items() if k < c.R[150 + li]}
    c.special |= set(range(40, 51)) | {230, 231}
    return c


def test_more_than_one_round(cols):
    kerns = cols([("rounds", rounds_case().lists(1))], 1, SOFT, 1, orc.MODE_COUNT, launches=2, pair=False)
    assert kerns[1] == "k_merge_cols"


@pytest.mark.parametrize("build", ["pa", "arena", "resc", "k63"])
def test_other_builds(cols, build):
    """the same walk in the other instantiations: presence/absence rows; count rows left in the arena (4-byte image, no NAR); share-min
    1 with soft-mins of 2 ... 4 over counts from 1 (RESC: records below the soft-min are set aside with a flag, or rescued); 128-bit
    keys (8 window slots, tiles of 56, one slice a tile).  Each over the marks of a whole wave, the middle split and the rounds."""
    if build == "k63":
        n = 262
        c = Case(63, 150, kw=2, n=n).sprinkle()
        for j in range(8):
            for h, row in enumerate((5, 30, 60, 90, 120)):
                c.run_after(128 + 24 + j, row, RUNS[(h + j) % 5], off=1 + 100 * j)
        c.hold_all(7)
        c.run_after(7, 70, 40)
        for d in (-1, 1):
            c.put(260, c.R[56] + d, 4)
            c.put(3, c.R[112] + d, 4)
        kerns = cols([("k63", c.lists(1))], 2, SOFT[:n], 1, orc.MODE_COUNT, launches=2, pair=False)
        assert kerns[1] == "k_merge_cols"
        return
    sets = [("marks-wave", marks_whole_wave().lists(1)), ("middle300", middle_case(300).lists(1)), ("rounds", rounds_case().lists(1))]
    if build == "pa":
        kerns = cols(sets, 1, SOFT, 1, orc.MODE_PA, launches=2, pair=False)
    elif build == "arena":
        kerns = cols(sets, 1, SOFT, 1, orc.MODE_COUNT, order=False, launches=2, pair=False)
    else:
        soft = [2 + (i % 3) for i in range(N)]
        c = Case(70, 300, count_lo=1, count_hi=9).sprinkle(phase=2)
        for j in range(8):
            for h, row in enumerate((10, 70, 130, 180, 240)):
                c.run_after(128 + 24 + j, row, RUNS[(h + j) % 5], count=1 + (h + j) % 4, off=1 + 100 * j)
        sets = [("resc-wave", c.lists(1))] + sets[1:]
        kerns = cols(sets, 1, soft, 1, orc.MODE_COUNT, share_min=1, launches=2, pair=False)
    assert kerns[1] == "k_merge_cols"
