"""The merge kernels over the whole key space and at extreme counts.  Every other merge test draws keys whose most significant word stays
below 2^62; real k-mers of k = 32, 64 and 96 fill that word (ceil(k / 32) words): a canonical k-mer that starts with G or T has a top
word of at least 2^63, and the largest canonical 64-mer's is all ones -- one word short of the sentinel the kernels use for an exhausted
cursor.  Here the keys of tests/synth.py's full-width shapes (around 2^63, at the largest canonical value, equal upper words with bit 63 of
the low word set and clear, keys 0 and 1) and counts up to 2^32 - 1 go through each forced kernel (the autouse fixture of
test_merge_gpu.py: k_merge_rows, k_merge_pivot, k_merge_cols + k_cols_sparse in file order and in arena order) at list counts at which
that kernel keeps the task, and the kernel that ran is asserted.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import orc
from synth import synth_wide_lists, SHAPES, U64
from test_merge_gpu import ctx, merge_kernel  # noqa: F401  (fixtures: the module's context, every test once per kernel)
from test_merge_independent import EXTREME_COUNTS

pytestmark = pytest.mark.gpu

# (recurrence-min, share-min): pivot's case (no rescue), rescue at and above the recurrence-min, recurrence-min 0 (rows of zeros)
RS = [(1, 0), (2, 0), (2, 2), (0, 2)]


def expected_kernel(kern, kw, n, rec_min, share_min, mode):
    """the kernel a forced KMX_MERGE_KERNEL hands a task to when the task is beyond it (kmx_merge_dev's selection): k_merge_pivot takes
    64-bit keys without share-min at recurrence-min >= 1; the column-blocked pair keys of one and two words, share-min above max(1,
    recurrence-min) on count rows only; the next one down otherwise.  The pair hands a task of two lists down whatever its keys (to
    k_merge_pivot from 513 lists on, to k_merge_rows below)"""
    pivot = kw == 1 and share_min == 0 and rec_min >= 1 and n <= 1024
    cols = kw <= 2 and (share_min <= max(1, rec_min) or mode == orc.MODE_COUNT)
    if kern == "cols" and cols:
        return "k_merge_cols" if n > 2 else handed_down(kw, n, rec_min, share_min)
    if kern in ("cols", "pivot") and pivot:
        return "k_merge_pivot"
    return "k_merge_rows"


def handed_down(kw, n, rec_min, share_min):
    """where a task the column-blocked pair handed back runs again"""
    return "k_merge_pivot" if kw == 1 and share_min == 0 and rec_min >= 1 and 512 < n <= 1024 else "k_merge_rows"


def merge_checked(ctx, lists, kw, soft, rec_min, share_min, mode):
    """one task through kmx_merge_dev (the lists on the device): rows, the body (ordered on the device and put together from the arena
    + row order on the host) and the six statistics equal to the oracle's, exactly.  -> the kernel that produced it"""
    torch = pytest.importorskip("torch")
    from kmtricks_amd import lib
    eb, er, es = orc.merge_matrix([(k.reshape(-1), c) for k, c in lists], kw, soft, rec_min, share_min, mode)
    recs = [torch.from_numpy(lib.pack_records(k, c, kw).view(np.int32)).cuda() for k, c in lists]
    torch.cuda.synchronize()
    res = ctx.merge_dev([dict(lists=[(r.data_ptr(), r.shape[0]) for r in recs], key_words=kw, soft_min=soft, rec_min=rec_min,
                              share_min=share_min, mode=mode)])
    try:
        res.wait()
        kern = res.kernel()
        what = (kern, kw, len(lists), rec_min, share_min, mode)
        assert res.rows() == er, what
        body = res.body()
        if body != eb:
            a, b = np.frombuffer(body, np.uint8), np.frombuffer(eb, np.uint8)
            bad = np.nonzero(a != b)[0] if len(a) == len(b) else [min(len(a), len(b))]
            raise AssertionError(f"{what}: body differs at {len(bad)} bytes, first at {bad[:8]}")
        assert res.body_from_arena() == eb, what
        assert np.array_equal(res.stats(), es), (what, res.stats(), es)
    finally:
        res.free()
    return kern, es


def cohort(seed, n, kw, shape, **kws):
    """similar lists (the cohorts the column-blocked pair and the pivot kernel are built for): ~1500 keys each"""
    pool = 1500 if n < 1000 else 60
    return synth_wide_lists(seed, n, pool, 0.95, 20 if n < 1000 else 2, kw=kw, shape=shape, **kws)


def _only_rows(merge_kernel, kw):
    if kw > 2 and merge_kernel != "rows":
        pytest.skip("keys of three and four words run on k_merge_rows whatever kernel is asked for: one run suffices")


@pytest.mark.parametrize("n", [2, 40, 200, "200-big", 300, 600])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kw", [1, 2, 3])
def test_full_width_keys(ctx, merge_kernel, monkeypatch, kw, shape, n):
    """every shape at k = 32 (one word), 64 (two) and 96 (three), count and PA rows, soft-mins that vary per list, recurrence-min 0 ... 2
    and share-min 0 and 2.  200 lists twice: k_merge_rows' small build (the default up to 256 lists of one and two words) and the large
    one (KMX_ROWS_SMALL=0)"""
    _only_rows(merge_kernel, kw)
    if n == "200-big":
        if merge_kernel != "rows" or kw > 2:
            pytest.skip("the large build of k_merge_rows only")
        monkeypatch.setenv("KMX_ROWS_SMALL", "0")
        n = 200
    lists = cohort(1000 * kw + 10 * SHAPES.index(shape) + n, n, kw, shape, count_max=8)
    soft = [1 + (i % 3) for i in range(n)]
    for rec_min, share_min in RS:
        for mode in (orc.MODE_COUNT, orc.MODE_PA):
            kern, _ = merge_checked(ctx, lists, kw, soft, rec_min, share_min, mode)
            assert kern == expected_kernel(merge_kernel, kw, n, rec_min, share_min, mode), (kern, rec_min, share_min, mode)


@pytest.mark.parametrize("n", [40, 300])
@pytest.mark.parametrize("shape", SHAPES)
def test_full_width_keys_of_four_words(ctx, merge_kernel, shape, n):
    """keys of four words (k = 97 ... 127) with the most significant word over 62 bits: no k-mer reaches it, the API takes it"""
    _only_rows(merge_kernel, 4)
    lists = cohort(4000 + 10 * SHAPES.index(shape) + n, n, 4, shape, count_max=8)
    soft = [1 + (i % 3) for i in range(n)]
    for rec_min, share_min in ((1, 0), (2, 2)):
        for mode in (orc.MODE_COUNT, orc.MODE_PA):
            assert merge_checked(ctx, lists, 4, soft, rec_min, share_min, mode)[0] == "k_merge_rows"


@pytest.mark.parametrize("shape", ["uniform", "near-max"])
def test_full_width_keys_beyond_2048_lists(ctx, merge_kernel, shape):
    """2049 lists of keys of three words (k = 96): k_merge_rows' build with 4096 record slots a tile"""
    _only_rows(merge_kernel, 3)
    n = 2049
    lists = cohort(2049 + SHAPES.index(shape), n, 3, shape, count_max=8)
    soft = [1 + (i % 3) for i in range(n)]
    for rec_min, share_min, mode in ((1, 0, orc.MODE_COUNT), (2, 2, orc.MODE_PA), (0, 0, orc.MODE_COUNT)):
        assert merge_checked(ctx, lists, 3, soft, rec_min, share_min, mode)[0] == "k_merge_rows"


def _above_2_63(lists, kw):
    return [(k[k[:, kw - 1] >= np.uint64(1 << 63)], c[k[:, kw - 1] >= np.uint64(1 << 63)]) for k, c in lists]


@pytest.mark.parametrize("where", ["below", "above"])
@pytest.mark.parametrize("n,kw", [(40, 1), (600, 1), (300, 2)])
def test_range_layout(ctx, merge_kernel, n, kw, where):
    """the pivot list (kmx_merge_dev takes the list of median length among lists 0, n/4, n/2, 3n/4 and n - 1: all of them here) holds keys
    of the top half only, every sixteenth list keys entirely below 2^62 ("below") or entirely above the pivot's, at the largest canonical
    values ("above"): the first or the last of k_range_bounds' ranges and of the pivot kernel's tiles (the open-ended one) hold no key of
    the pivot list.  (Few and short enough that the lists stay a cohort: the column-blocked pair and the pivot kernel hand a task down
    when more than an eighth of its solid records lie outside the keys they take their rows from.  The column-blocked pair hands such a
    cohort down -- a list that shares no key with the others fills its set-aside slices, as in test_merge_gpu.py::test_cols_outlier_samples
    -- so under it the layout checks the chain cols -> pivot -> rows, and only the other two kernels are asserted by name.)"""
    from kmtricks_amd import lib
    top = _above_2_63(cohort(500 + n, n, kw, "straddle", count_max=8), kw)
    if where == "below":
        other = [(k[k[:, kw - 1] < np.uint64(1 << 62)], c[k[:, kw - 1] < np.uint64(1 << 62)]) for k, c in cohort(501 + n, n, kw, "uniform", count_max=8)]
    else:
        other = [(k[::2], c[::2]) for k, c in cohort(502 + n, n, kw, "near-max", count_max=8)]
    cand = {0, n // 4, n // 2, (3 * n) // 4, n - 1}
    lists = [other[i] if i % 16 == 3 and i not in cand else top[i] for i in range(n)]
    assert min(len(lists[i][0]) for i in cand) > 100
    soft = [1 + (i % 3) for i in range(n)]
    c = lib.Context(0)          # (the file order of the fixture's environment)
    try:
        for rec_min, share_min in ((1, 0), (2, 0), (1, 1)):
            for mode in (orc.MODE_COUNT, orc.MODE_PA):
                kern, _ = merge_checked(c, lists, kw, soft, rec_min, share_min, mode)
                if merge_kernel != "cols":
                    assert kern == expected_kernel(merge_kernel, kw, n, rec_min, share_min, mode), (kern, rec_min, share_min, mode)
    finally:
        c.close()


@pytest.mark.parametrize("n", [2, 200, 600])
@pytest.mark.parametrize("kw", [1, 2, 3])
def test_extreme_counts(ctx, merge_kernel, kw, n):
    """counts of 254, 255, 256, 65535, 65536, 2^31 and 2^32 - 1 sprinkled over every list; every third record of list 1 solid at 2^32 - 1
    (its TOTAL_WO and TOTAL_W pass 2^32, and so does the share of every lane of a window); list 0 with a soft-min of 2^32 - 1, so that none
    of its records is solid and with share-min on its TOTAL_W (statistic 5) is the sum of its rescued counts alone, past 2^32 too"""
    _only_rows(merge_kernel, kw)
    lists = cohort(7000 + 10 * kw + n, n, kw, "uniform", count_max=8)
    rng = np.random.default_rng(n + kw)
    edge = np.array(EXTREME_COUNTS, np.uint32)
    for _, c in lists:
        m = rng.random(len(c)) < 0.03
        c[m] = edge[rng.integers(0, len(edge), int(m.sum()))]
    lists[1][1][::3] = 0xFFFFFFFF
    lists[0][1][::2] = 0xFFFFFFFE
    lists[0][1][lists[0][1] == 0xFFFFFFFF] = 0xFFFFFFFE
    soft = [1 + (i % 3) for i in range(n)]
    soft[0] = 0xFFFFFFFF
    for rec_min, share_min in RS:
        for mode in (orc.MODE_COUNT, orc.MODE_PA):
            kern, es = merge_checked(ctx, lists, kw, soft, rec_min, share_min, mode)
            assert kern == expected_kernel(merge_kernel, kw, n, rec_min, share_min, mode), (kern, rec_min, share_min, mode)
            assert es[4][1] > 1 << 34 and es[5][1] > 1 << 34 and es[4][0] == 0
            if share_min and n > 2:
                assert es[5][0] > 1 << 33          # (rescued counts alone)


@pytest.mark.parametrize("n,kw", [(2, 1), (40, 1), (300, 1), (40, 2), (300, 2), (40, 3)])
def test_all_ones_key(ctx, merge_kernel, n, kw):
    """a key of all ones (every word ~0: no canonical k-mer, the value the kernels use for an exhausted cursor, a pad or an open tile
    limit) is a key like any other to the reference's merger: in most lists, solid in some, non-solid in others, next to the largest
    canonical keys"""
    _only_rows(merge_kernel, kw)
    lists = cohort(9000 + 10 * kw + n, n, kw, "near-max", count_max=8)
    ones = np.full((1, kw), U64, np.uint64)
    rng = np.random.default_rng(n)
    for i in range(n):
        if i % 5 != 4:
            k, c = lists[i]
            lists[i] = (np.concatenate([k, ones]), np.concatenate([c, rng.integers(1, 5, 1).astype(np.uint32)]))
    soft = [1 + (i % 3) for i in range(n)]
    for rec_min, share_min in RS:
        for mode in (orc.MODE_COUNT, orc.MODE_PA):
            kern, _ = merge_checked(ctx, lists, kw, soft, rec_min, share_min, mode)
            assert kern == expected_kernel(merge_kernel, kw, n, rec_min, share_min, mode), (kern, rec_min, share_min, mode)


def test_stress_scripts_with_full_width_keys(merge_kernel):
    """scripts/stress_cols.py and scripts/stress_merge.py with "wide": about half of their random cases draw keys of tests/synth.py's
    full-width shapes (the column-blocked pair forced, keys of one and two words; libkmx's own choice over count / PA / Bloom rows)"""
    import os, subprocess, sys
    if merge_kernel != "cols":
        pytest.skip("one run is enough")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env.pop("KMX_MERGE_KERNEL", None); env.pop("KMX_ITEMS_PER_SLOT", None)
    for script, args, n in (("stress_cols.py", ["wide"], 12), ("stress_cols.py", ["cols", "kw2", "wide"], 8), ("stress_merge.py", ["wide"], 12)):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", script), str(n), "31"] + args, capture_output=True, text=True, env=env)
        assert r.returncode == 0 and f"all {n} cases equal the oracle" in r.stdout, (script, args, r.stdout[-1500:] + r.stderr[-1500:])
        assert any(f"keys={s} " in r.stdout for s in SHAPES), (script, args)      # (some case did draw full-width keys)
