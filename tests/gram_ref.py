"""The definition of `kmx pca`'s device table (include/kmx.h, section "gram") restated for the tests, by two roads that share no code:
plain Python integers a row and a pair at a time (gram_expected_py) and numpy a recurrence class at a time (gram_expected_np).  Beside
them the driver's class weights, its fixed point F and its Gram matrix in exact fractions.Fraction, the driver's texts, and the list of
bodies and parameters that tests/test_gram_gpu.py sends to the device."""
import functools
import struct
from fractions import Fraction

import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload, make_body, write_run, read_run_bodies  # noqa: F401
from pan_ref import make_cols, shaped_body  # noqa: F401

U32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


# ---- road 1: Python integers, a row and a pair at a time --------------------------------------------------------------------------
def gram_expected_py(body, n_cols, key_words, mode, weights, cols=None, min_abund=1):
    """-> n_cols lists of n_cols integers, modulo 2^64"""
    raw, rb, N = as_bytes(body), row_bytes(key_words, n_cols, mode), n_cols
    assert len(raw) % rb == 0
    cols = list(range(N)) if cols is None else [int(c) for c in cols]
    assert len(weights) == len(cols) + 1
    T = [[0] * N for _ in range(N)]
    for r in range(len(raw) // rb):
        pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
        held = []
        for c in cols:
            if mode == MODE_COUNT:
                if struct.unpack_from("<I", pay, 4 * c)[0] >= min_abund:
                    held.append(c)
            elif (pay[c >> 3] >> (c & 7)) & 1:
                held.append(c)
        w = int(weights[len(held)])
        if not w:
            continue
        for i in held:
            row = T[i]
            for j in held:
                row[j] = (row[j] + w) & MASK64
    return T


# ---- road 2: numpy, a recurrence class at a time ----------------------------------------------------------------------------------
def presence(body, n_cols, key_words, mode, cols=None, min_abund=1):
    """-> bool [rows, M] in list order"""
    cols = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    pay = split_payload(body, n_cols, key_words, mode)[:, cols]
    return pay >= min_abund if mode == MODE_COUNT else pay.astype(bool)


def gram_expected_np(body, n_cols, key_words, mode, weights, cols=None, min_abund=1):
    """-> uint64 [n_cols, n_cols].  A class's co-presence counts are a float64 product (exact: a count is below 2^53), times the class's
    weight in uint64, which wraps modulo 2^64 as the device's adds do"""
    ci = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    M = len(ci)
    weights = np.asarray(weights, np.uint64)
    assert len(weights) == M + 1
    present = presence(body, n_cols, key_words, mode, cols, min_abund)
    assert len(present) < 2 ** 31
    rec = present.sum(axis=1).astype(np.int64)
    in_list = np.zeros((M, M), np.uint64)
    for r in np.unique(rec):
        if weights[r]:
            B = present[rec == r].astype(np.float64)
            in_list += (B.T @ B).astype(np.uint64) * weights[r]
    T = np.zeros((n_cols, n_cols), np.uint64)
    T[np.ix_(ci, ci)] = in_list
    return T


def class_sizes(body, n_cols, key_words, mode, cols=None, min_abund=1):
    M = n_cols if cols is None else len(cols)
    return np.bincount(presence(body, n_cols, key_words, mode, cols, min_abund).sum(axis=1).astype(np.int64), minlength=M + 1)


def words_used(sizes, weights):
    """Wu: the 64-row words of the recurrence order -- a class of a weight other than 0 starts on a word"""
    return sum((int(n) + 63) // 64 for n, w in zip(sizes, weights) if int(w))


# ---- the driver, exact ------------------------------------------------------------------------------------------------------------
def driver_weights(M, n, scale="eigenstrat", min_rec=1, max_rec=None):
    """-> (wt: M + 1 integers, F, n_used) as `kmx pca` chooses them from the spectrum n (rows by recurrence); None when nothing fits"""
    lo, hi = max(1, min_rec), min(M - 1, M if max_rec is None else max_rec)
    for F in (range(31, -1, -1) if scale == "eigenstrat" else [0]):
        wt = [0] * (M + 1)
        for R in range(lo, hi + 1):
            d = R * (M - R)
            wt[R] = ((1 << (F + 1)) * M * M + d) // (2 * d) if scale == "eigenstrat" else 1
        if max(wt) <= U32 and sum(w * int(x) for w, x in zip(wt, n)) < 2 ** 63:
            return wt, F, sum(int(x) for w, x in zip(wt, n) if w)
    return None


def gram_exact(M, cols, wt, F, n, sh, T):
    """G [M][M] in list order as Fractions, and per cell the magnitude (T_ij 2^-F + A_i + A_j + S) / n_used the driver's rounding bound is
    a multiple of.  n: rows by recurrence; sh [M + 1][N] and T [N][N] by input column"""
    cols = list(range(M)) if cols is None else [int(c) for c in cols]
    n_used = sum(int(n[R]) for R in range(M + 1) if wt[R])
    w = [Fraction(wt[R], 1 << F) for R in range(M + 1)]
    A = [sum(w[R] * Fraction(R, M) * int(sh[R][c]) for R in range(M + 1) if wt[R]) for c in cols]
    S = sum(w[R] * Fraction(R * R, M * M) * int(n[R]) for R in range(M + 1) if wt[R])
    G = [[None] * M for _ in range(M)]
    mag = [[None] * M for _ in range(M)]
    for i in range(M):
        for j in range(M):
            t = Fraction(int(T[cols[i]][cols[j]]), 1 << F)
            G[i][j] = (t - A[i] - A[j] + S) / n_used
            mag[i][j] = (t + A[i] + A[j] + S) / n_used
    return G, mag


# ---- the driver's texts -----------------------------------------------------------------------------------------------------------
def gram_text(ids, G):
    lines = ["# kmx pca gram", f"# samples: {len(ids)}"] + [f"# id: {s}" for s in ids]
    lines += ["\t".join("%.17g" % float(v) for v in row) for row in G]
    return "\n".join(lines) + "\n"


def parse_gram(text):
    lines = text.splitlines()
    assert lines[0] == "# kmx pca gram" and lines[1].startswith("# samples: ")
    M = int(lines[1][11:])
    ids = [ln[6:] for ln in lines[2:2 + M]]
    assert all(ln.startswith("# id: ") for ln in lines[2:2 + M]) and len(lines) == 2 + 2 * M
    G = np.array([[float(x) for x in ln.split("\t")] for ln in lines[2 + M:]])
    assert G.shape == (M, M)
    return ids, G


def parse_pcs(text):
    """-> (ids, float [M, k])"""
    lines = text.splitlines()
    head = lines[0].split("\t")
    assert head[0] == "sample" and head[1:] == [f"PC{c}" for c in range(1, len(head))]
    cells = [ln.split("\t") for ln in lines[1:]]
    assert all(len(c) == len(head) for c in cells)
    return [c[0] for c in cells], np.array([[float(x) for x in c[1:]] for c in cells]).reshape(len(cells), len(head) - 1)


# ---- what the GPU test sends ------------------------------------------------------------------------------------------------------
def classed_body(seed, sizes, N, kw, mode, cols=None, maxed=0.05):
    """rows with exactly sizes[R] rows of recurrence R over the list, in random order; the unlisted columns are held at random (they
    must not reach the table).  COUNT: counts 1 ... 3, a share `maxed` 2^32 - 1; PA: every padding bit set"""
    rng = np.random.default_rng(seed)
    ci = np.arange(N) if cols is None else np.asarray(cols, np.int64)
    M = len(ci)
    assert len(sizes) == M + 1
    recs = rng.permutation(np.repeat(np.arange(M + 1), np.asarray(sizes, np.int64)))
    n_rows = len(recs)
    held = rng.random((n_rows, N)) < 0.5
    held[:, ci] = np.argsort(rng.random((n_rows, M)), axis=1) < recs[:, None]
    keys = rng.integers(0, 256, (n_rows, 8 * kw), dtype=np.uint8)
    if mode == MODE_COUNT:
        c = rng.integers(1, 4, (n_rows, N)).astype(np.uint32)
        c[rng.random((n_rows, N)) < maxed] = U32
        c[~held] = 0
        pay = c.astype("<u4").view(np.uint8).reshape(n_rows, 4 * N)
    else:
        bits = np.concatenate([held, np.ones((n_rows, (-N) % 8), bool)], axis=1)
        pay = np.packbits(bits, axis=1, bitorder="little").reshape(n_rows, (N + 7) // 8)
    return np.ascontiguousarray(np.concatenate([keys, pay], axis=1)).reshape(-1)


def make_weights(kind, M, seed=0):
    """the weight shapes of the sweep -> uint32 [M + 1]"""
    w = np.ones(M + 1, np.uint32)
    if kind == "ones":
        return w
    if kind == "max":
        return np.full(M + 1, U32, np.uint32)
    if kind == "dist":            # identity (b) of the header: the table is inter of kmx_dist_*
        w[0] = 0
        return w
    if kind == "holes":           # zero for some classes, the largest and the class of every second recurrence among them
        w = np.random.default_rng(seed).integers(1, 2 ** 32, M + 1, dtype=np.uint64).astype(np.uint32)
        w[::2] = 0
        w[M] = 0
        return w
    assert kind == "eigenstrat"   # the driver's own at F = 8: large next to the ends, zero at them
    w = np.zeros(M + 1, np.uint32)
    for R in range(1, M):
        w[R] = min(U32, ((1 << 9) * M * M + R * (M - R)) // (2 * R * (M - R)))
    return w


class Case:
    def __init__(self, name, mode, n_cols, key_words, n_rows, cols, abund, weights, make):
        self.name, self.mode, self.n_cols, self.key_words, self.n_rows, self.cols, self.abund, self.weights, self._make = name, mode, n_cols, key_words, n_rows, cols, abund, weights, make
        self.n_use = n_cols if cols is None else len(cols)

    @functools.cached_property
    def body(self):
        b = self._make()
        assert len(b) == self.n_rows * row_bytes(self.key_words, self.n_cols, self.mode)
        b.setflags(write=False)
        return b

    @functools.cached_property
    def expected(self):
        """the numpy road's word, worked out once"""
        t = gram_expected_np(self.body, self.n_cols, self.key_words, self.mode, self.weights, self.cols, self.abund)
        t.setflags(write=False)
        return t

    @functools.cached_property
    def words(self):
        return words_used(class_sizes(self.body, self.n_cols, self.key_words, self.mode, self.cols, self.abund), self.weights)


COLUMNS = [1, 7, 63, 64, 65, 130, 513]      # a byte, a block of 64 samples, several block pairs, a PA lane's span of 512 columns
ROWS = [0, 1, 63, 64, 65, 700, 12001]       # a word, a tile, several runs a block pair
SHAPES = ["same", "uniform", "skewed", 0.5]
KINDS = ["none", "reversed", "scattered", "one"]
WEIGHTS = ["ones", "max", "holes", "eigenstrat", "dist"]
ABUNDS = [1, 2, U32]


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """combinations, not the full product: every N in both modes and every value of the other axes -- they rotate at strides that are
    coprime to each other (test_gram_cpu asserts the coverage)"""
    cases = []

    def add(name, mode, N, kw, rows, cols, a, wkind, make):
        M = N if cols is None else len(cols)
        cases.append(Case(name, mode, N, kw, rows, cols, a, make_weights(wkind, M, 31 + len(cases)), make))

    i = 0
    for N in COLUMNS:
        for mode in (MODE_COUNT, MODE_PA):
            for rep in range(3):
                rows = ROWS[(i * 3 + rep) % len(ROWS)]
                if mode == MODE_COUNT and N >= 513 and rows > 700:
                    rows = 700      # (the long bodies ride on narrower matrices: a few MB at the most)
                kw = 1 + (i // 2 + i) % 4
                shape = SHAPES[(i + rep) % len(SHAPES)]
                kind = KINDS[(i + rep) % len(KINDS)]
                wkind = WEIGHTS[(i * 2 + rep) % len(WEIGHTS)]
                sd = 7000 + 10 * i + rep
                cols = make_cols(kind, N, sd)
                a = ABUNDS[(i + rep) % 3] if mode == MODE_COUNT else 1
                make = (lambda sd=sd, rows=rows, N=N, kw=kw, mode=mode, shape=shape: shaped_body(sd, rows, N, kw, mode, shape))
                m = "c" if mode == MODE_COUNT else "p"
                add(f"{m}-{N}-{kind}-r{rows}-k{kw}-{shape}-{wkind}-a{a}", mode, N, kw, rows, cols, a, wkind, make)
            i += 1
    # one wide matrix: more than one trip of a PA lane, 17 sample blocks
    for mode in (MODE_COUNT, MODE_PA):
        make = (lambda mode=mode: shaped_body(7900, 300, 1025, 2, mode, "uniform"))
        add(f"{'c' if mode == MODE_COUNT else 'p'}-1025-scattered-r300-k2-uniform-eigenstrat-a1", mode, 1025, 2, 300, make_cols("scattered", 1025, 7900), 1, "eigenstrat", make)
    # the padding edge: classes of exactly 63, 64 and 65 rows (and of 1, 128 and 129), every other class empty; the list scattered, so
    # that unlisted columns are held too
    for mode in (MODE_COUNT, MODE_PA):
        for N, kind, wkind in ((9, "none", "ones"), (70, "scattered", "max"), (130, "reversed", "holes"), (65, "scattered", "eigenstrat")):
            sd = 8000 + len(cases)
            cols = make_cols(kind, N, sd)
            M = N if cols is None else len(cols)
            sizes = [0] * (M + 1)
            for R, n in zip(range(1, M + 1), (63, 64, 65, 1, 128, 129, 64, 63)):
                sizes[R] = n
            sizes[0] = 5
            make = (lambda sd=sd, sizes=tuple(sizes), N=N, mode=mode, cols=cols: classed_body(sd, sizes, N, 1 + sd % 4, mode, cols))
            add(f"{'c' if mode == MODE_COUNT else 'p'}-{N}-{kind}-r{sum(sizes)}-k{1 + sd % 4}-edge-{wkind}-a1", mode, N, 1 + sd % 4, sum(sizes), cols, 1, wkind, make)
    # every class present, long: several runs a block pair and a weight change in most panels
    for mode in (MODE_COUNT, MODE_PA):
        make = (lambda mode=mode: shaped_body(8100, 12001, 65, 1, mode, "uniform"))
        add(f"{'c' if mode == MODE_COUNT else 'p'}-65-none-r12001-k1-uniform-max-a1-long", mode, 65, 1, 12001, None, 1, "max", make)
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
