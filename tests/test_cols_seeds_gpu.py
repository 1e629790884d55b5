"""k_cols_seeds + the row tables k_merge_cols fills from its hash words: the column-blocked pair against the CPU oracle at the
smallest shapes where a tile's hash word, the table that is never cleared between the tiles of a work item, or the hand-back
of a task without a word can go wrong.  520 lists (five column blocks; count rows in file order take the byte-wide NAR build),
tiles of 112 row keys (56 for 128-bit keys).  Needs an MI355X: run with -m gpu.

How many tiles a work item walks is libkmx's choice (key ranges per task = work items wanted / tasks of the batch / column
blocks): BATCH tasks over the same device lists with KMX_ITEMS_PER_SLOT=1 leave every task ONE key range, so a work item walks
all the tiles of the pool -- 1, 2, 3 and 5 for pools of 100, 224, 300 and 460 keys; with KMX_ITEMS_PER_SLOT=3 a task has two
ranges and a workgroup switches between items of a few tiles each."""
import numpy as np
import pytest

import orc
from synth import synth_lists, _assemble

pytestmark = pytest.mark.gpu
N = 520
BATCH = 64
_oracle = {}


def expected(tag, lists, kw, soft, rec_min, mode):
    """the oracle's (body, rows, stats) of a set of lists, computed once per module"""
    key = (tag, kw, rec_min, mode)
    if key not in _oracle:
        _oracle[key] = orc.merge_matrix([(k.reshape(-1), c) for k, c in lists], kw, soft, rec_min, 0, mode)
    return _oracle[key]


_lists = {}


def p_present(pool):
    """the share of the pool a list holds.  The row keys come from a merge of 8 of the lists in key ranges of total / 1500 records,
    each sorted in LDS 2048 records at a time: 8 lists of 2049 to 2999 records in all are one range that does not fit, and the
    pair hands the task back before it starts -- lists of 257 to 374 records, what 0.97 of a pool of 300 gives.  0.8 of it (246
    records a list) still makes every pool key a row key (a key is missing from 7 of the 8 lists once in 12000 times)."""
    return 0.8 if 257 <= 0.97 * pool + 6 <= 374 else 0.97


def pool_lists(pool, kw=1, n=N):
    key = (pool, kw, n)
    if key not in _lists:
        _lists[key] = synth_lists(4200 + pool + n, n, pool, p_present(pool), 6, kw=kw, key_bits=62 if kw == 1 else 100, count_max=200)
    return _lists[key]


@pytest.fixture
def cols(monkeypatch):
    """-> run(sets, kw, soft, rec_min, mode, order=True, ...): one batch through the pair, every task against the oracle"""
    torch = pytest.importorskip("torch")
    from kmtricks_amd import lib
    monkeypatch.setenv("KMX_MERGE_KERNEL", "cols")
    monkeypatch.setenv("KMX_FILE_ORDER", "1")
    made = []

    def run(sets, kw, soft, rec_min, mode, order=True, batch=1, per_slot=None, tries=None, pair=True, launches=1):
        """sets: [(tag, lists)]: the batch is every set `batch` times over (the same device lists), merged `launches` times on one
        context; -> the kernel of the last launch"""
        monkeypatch.setenv("KMX_FILE_ORDER", "1" if order else "0")
        if per_slot is not None:
            monkeypatch.setenv("KMX_ITEMS_PER_SLOT", str(per_slot))
        if tries is not None:
            monkeypatch.setenv("KMX_COLS_SEED_TRIES", str(tries))
        ctx = lib.Context(0)
        made.append(ctx)
        ctx.set_file_order(order)
        tasks, exp, keep = [], [], []
        for tag, lists in sets:
            recs = [torch.from_numpy(lib.pack_records(k, c, kw).view(np.int32)).cuda() for k, c in lists]
            keep.append(recs)
            t = dict(lists=[(r.data_ptr(), r.shape[0]) for r in recs], key_words=kw, soft_min=soft, rec_min=rec_min, share_min=0, mode=mode)
            tasks += [t] * batch
            exp += [expected(tag, lists, kw, soft, rec_min, mode)] * batch
        torch.cuda.synchronize()
        for _ in range(launches):
            res = ctx.merge_dev(tasks)
            res.wait()
            kern = res.kernel()
            for t, (eb, er, es) in enumerate(exp):
                assert res.rows(t) == er, (t, res.rows(t), er)
                assert res.body(t) == eb, f"task {t}: body differs"
                assert np.array_equal(res.stats(t), es), t
            res.free()
        if pair:
            assert kern == "k_merge_cols"
        return kern

    yield run
    for c in made:
        c.close()


SOFT = [1 + (i % 2) for i in range(N)]


@pytest.mark.parametrize("per_slot", [1, 3])
@pytest.mark.parametrize("pool", [100, 224, 300, 460])
def test_tiles_per_work_item(cols, pool, per_slot):
    """1, 2, 3 and 5 tiles: both parities of the table in turn, a ragged last tile; BATCH tasks with the same keys, so every
    workgroup meets the same keys again in its next item (with a table left over from the last one they would hit)"""
    cols([(f"pool{pool}", pool_lists(pool))], 1, SOFT, 2, orc.MODE_COUNT, batch=BATCH, per_slot=per_slot)


def test_same_keys_in_consecutive_items_other_rows(cols):
    """two tasks side by side: the second holds the first one's lists, but 40 of the shared keys are left in ONE list only -- row
    keys of the first task, private k-mers of the second.  An entry of the first task's table that outlived its work item would
    take those records for row keys' records."""
    a = pool_lists(300)
    rng = np.random.default_rng(5)
    keys, held = np.unique(np.concatenate([k[:, 0] for k, _ in a]), return_counts=True)
    drop = rng.choice(keys[held > N // 2], 40, replace=False)      # (shared keys: row keys of the first task)
    b = []
    for i, (k, c) in enumerate(a):
        m = np.ones(len(c), bool) if i == 3 else ~np.isin(k[:, 0], drop)
        b.append((np.ascontiguousarray(k[m]), np.ascontiguousarray(c[m])))
    cols([("pool300", a), ("pool300-drop", b)] * 8, 1, SOFT, 2, orc.MODE_COUNT, per_slot=1, batch=4)


def test_tile_the_cheap_hashes_cannot_split(cols):
    """row keys in pairs x, x + 2^58 inside one tile: the 64 cheap hash words fold key bits below 55 only, so every one of them
    puts a pair into one entry -- the tiles take words of the 64-bit family, and no task is handed back"""
    rng = np.random.default_rng(58)
    low = np.unique(rng.integers(0, 1 << 55, 170, dtype=np.uint64))[:150].reshape(3, 50)
    shared = np.concatenate([np.concatenate([low[t] | np.uint64(t << 60), low[t] | np.uint64(t << 60) | np.uint64(1 << 58)]) for t in range(3)])
    priv = np.unique(rng.integers(0, 1 << 62, N * 6 + 400, dtype=np.uint64))
    priv = priv[~np.isin(priv, shared)]
    rng.shuffle(priv)
    allk = np.concatenate([shared, priv[:N * 6]]).reshape(-1, 1)
    lists = _assemble(rng, allk, N, len(shared), p_present(len(shared)), 6, 1, 200)
    cols([("pairs58", lists)], 1, SOFT, 2, orc.MODE_COUNT, batch=BATCH, per_slot=1)


def test_no_hash_word_hands_the_task_back(cols):
    """KMX_COLS_SEED_TRIES=1: 112 keys land in distinct entries of 4096 under the first word for a tile in five (e^(-112 * 111 / 8192)
    = 0.22), so a task of four full tiles keeps all its words once in 400 times: the tasks are handed back before k_merge_cols
    starts on them, and the next kernel down completes them"""
    kern = cols([("pool460", pool_lists(460))], 1, SOFT, 2, orc.MODE_COUNT, batch=BATCH, per_slot=1, tries=1, pair=False)
    assert kern != "k_merge_cols"


def test_big_counts_in_consecutive_tiles(cols):
    """counts of 254, 255, 256 and 2^32-1 over a third of all records, five tiles a work item: the rows' flags of both parities"""
    lists = [(k, c.copy()) for k, c in pool_lists(460)]
    rng = np.random.default_rng(460)
    edge = np.array([254, 255, 256, 0xFFFFFFFF], dtype=np.uint32)
    for _, c in lists:
        m = rng.random(len(c)) < 0.3
        c[m] = edge[rng.integers(0, len(edge), int(m.sum()))]
    cols([("pool460-big", lists)], 1, SOFT, 2, orc.MODE_COUNT, batch=BATCH, per_slot=1)


def test_further_rounds_in_a_tile(cols):
    """a list with 300 private keys between two neighbouring row keys -- more than its window of 128: that tile takes further rounds.
    They are also more than the 128 entries of a wave's set-aside slice: the first launch of a context hands such tasks back (and
    is checked like any other), the context's next launch runs the build whose waves claim slice extensions and completes them."""
    lists = list(pool_lists(300))
    k, c = lists[4]
    lo = int(k[len(k) // 2, 0])
    run = (np.arange(1, 301, dtype=np.uint64) + np.uint64(lo)).reshape(-1, 1)
    taken = np.concatenate([x[:, 0] for x, _ in lists])
    run = run[~np.isin(run[:, 0], taken)]
    assert len(run) > 290
    k2 = np.concatenate([k, run]); c2 = np.concatenate([c, np.full(len(run), 3, np.uint32)])
    o = np.argsort(k2[:, 0]); lists[4] = (np.ascontiguousarray(k2[o]), np.ascontiguousarray(c2[o]))
    cols([("pool300-run", lists)], 1, SOFT, 2, orc.MODE_COUNT, batch=BATCH, per_slot=1, launches=2)


@pytest.mark.parametrize("build", ["arena", "pa", "k63"])
@pytest.mark.parametrize("pool", [224, 460])
def test_builds_with_two_barriers(cols, build, pool):
    """the builds that keep a barrier on either side of the tile's way out use the same hash words: count rows where the kernels
    leave them (4-byte image), presence/absence rows, and 262 lists of 128-bit keys (tiles of 56 row keys, 2048-entry table)"""
    if build == "k63":
        n = 262
        cols([(f"k63-{pool}", pool_lists(pool, 2, n))], 2, SOFT[:n], 2, orc.MODE_COUNT, batch=BATCH, per_slot=1)
    elif build == "pa":
        cols([(f"pool{pool}", pool_lists(pool))], 1, SOFT, 2, orc.MODE_PA, batch=BATCH, per_slot=1)
    else:
        cols([(f"pool{pool}", pool_lists(pool))], 1, SOFT, 2, orc.MODE_COUNT, order=False, batch=BATCH, per_slot=1)
