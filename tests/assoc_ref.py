"""The definition of `kmx assoc`'s device call (include/kmx.h, section "assoc") restated for the tests, by two roads that share no code:
plain Python integers and floats a row at a time (assoc_expected_py) and numpy, the bit matrix times the vector table in int64 and the
formula elementwise in float64 (assoc_expected_np).  Both keep the order of operations the header writes down, and neither a Python float
nor a numpy elementwise operation fuses a multiply with an add: their stat and beta are held bit for bit against each other and against
the device.  Beside them the list of bodies and parameters that tests/test_assoc_gpu.py sends to the device."""
import functools
import math
import struct

import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload, make_body, write_run, read_run_bodies  # noqa: F401
from pan_ref import shaped_body  # noqa: F401

U32 = 0xFFFFFFFF
INF = float("inf")
# kmx_assoc_rec
REC = np.dtype([("stat", "<f8"), ("beta", "<f8"), ("s0", "<i8"), ("rec", "<u4"), ("row", "<u4")])
VP_STEPS = (1, 2, 4, 8, 12, 16, 24, 32)      # the vector counts k_assoc_score is built for: V rides on the smallest at or above it


# ---- road 1: Python integers and floats, a row at a time --------------------------------------------------------------------------
def assoc_rows_py(body, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, cols=None, min_abund=1):
    """-> a list of (rec, s0, stat, beta), one per input row"""
    raw, rb, N = as_bytes(body), row_bytes(key_words, n_cols, mode), n_cols
    assert len(raw) % rb == 0
    cols = list(range(N)) if cols is None else [int(c) for c in cols]
    vecs = [[int(x) for x in row] for row in vecs]
    assert len(vecs) == len(cols)
    V = len(vecs[0])
    sc = math.ldexp(1.0, -frac_bits)
    out = []
    for r in range(len(raw) // rb):
        pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
        s = [0] * V
        rec = 0
        for m, c in enumerate(cols):
            if mode == MODE_COUNT:
                here = struct.unpack_from("<I", pay, 4 * c)[0] >= min_abund
            else:
                here = (pay[c >> 3] >> (c & 7)) & 1
            if here:
                rec += 1
                row = vecs[m]
                for j in range(V):
                    s[j] += row[j]
        assert all(abs(x) < 2 ** 53 for x in s)
        u = float(s[0]) * sc
        h = 0.0
        for j in range(1, V):
            a = float(s[j]) * sc
            h = h + a * a
        v = float(rec) - h
        if v > vmin:
            beta = u / v
            stat = (gain * (u * u)) / v
        else:
            beta = 0.0
            stat = 0.0
        out.append((rec, s[0], stat, beta))
    return out


def assoc_expected_py(body, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols=None, min_abund=1, min_rec=0, max_rec=U32):
    """-> the records of the kept rows, in input order: a list of (stat, beta, s0, rec, row)"""
    rows = assoc_rows_py(body, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, cols, min_abund)
    return [(stat, beta, s0, rec, i) for i, (rec, s0, stat, beta) in enumerate(rows) if min_rec <= rec <= max_rec and stat >= threshold]


# ---- road 2: numpy, the whole body at once ----------------------------------------------------------------------------------------
def presence(body, n_cols, key_words, mode, cols=None, min_abund=1):
    """-> bool [rows, M] in list order"""
    cols = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    pay = split_payload(body, n_cols, key_words, mode)[:, cols]
    return pay >= min_abund if mode == MODE_COUNT else pay.astype(bool)


def assoc_rows_np(body, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, cols=None, min_abund=1):
    """-> a REC array with one entry per input row"""
    X = presence(body, n_cols, key_words, mode, cols, min_abund).astype(np.int64)
    vt = np.asarray(vecs, np.int64)
    assert vt.ndim == 2 and vt.shape[0] == X.shape[1]
    assert np.abs(vt).sum(axis=0).max() < 2 ** 53
    S = X @ vt                                     # int64 [rows, V]: exact
    rec = X.sum(axis=1)
    sc = np.float64(2.0) ** -frac_bits
    u = S[:, 0].astype(np.float64) * sc
    h = np.zeros(len(X), np.float64)
    for j in range(1, vt.shape[1]):
        a = S[:, j].astype(np.float64) * sc
        h = h + a * a
    v = rec.astype(np.float64) - h
    ok = v > vmin
    vs = np.where(ok, v, 1.0)
    out = np.zeros(len(X), REC)
    out["stat"] = np.where(ok, (np.float64(gain) * (u * u)) / vs, 0.0)
    out["beta"] = np.where(ok, u / vs, 0.0)
    out["s0"], out["rec"], out["row"] = S[:, 0], rec, np.arange(len(X))
    return out


def assoc_expected_np(body, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols=None, min_abund=1, min_rec=0, max_rec=U32):
    """-> (the kept rows' records as a REC array in input order, the kept rows' bytes)"""
    allr = assoc_rows_np(body, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, cols, min_abund)
    keep = (allr["rec"] >= min_rec) & (allr["rec"] <= max_rec) & (allr["stat"] >= threshold)
    rb = row_bytes(key_words, n_cols, mode)
    rows = np.frombuffer(as_bytes(body), np.uint8).reshape(-1, rb)
    return allr[keep], rows[keep].tobytes()


def algo_bytes(n_rows, n_cols, key_words, mode, n_vec, kept):
    rb = row_bytes(key_words, n_cols, mode)
    return n_rows * rb + kept * (rb + 32) + 4 * n_cols * n_vec


def same_bits(a, b):
    """float64 arrays equal bit for bit"""
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- what the GPU test sends ------------------------------------------------------------------------------------------------------
def make_cols(kind, N, seed):
    """the lists of the sweep -> a uint32 array, or None (the identity said by leaving the list out)"""
    if kind == "none":
        return None
    if kind == "one":
        return np.array([N // 2], np.uint32)
    if kind == "second":
        return np.arange(0, N, 2, dtype=np.uint32)
    assert kind == "subset"          # a permuted subset
    return np.random.default_rng(seed).permutation(N)[:max(1, (2 * N) // 3)].astype(np.uint32)


def make_vecs(kind, M, V, seed):
    """the vector tables of the sweep -> int32 [M, V]"""
    rng = np.random.default_rng(seed)
    if kind == "pos":                # a 32-bit partial sum wraps from the second present column on
        return np.full((M, V), 2 ** 30, np.int32)
    if kind == "neg":
        return np.full((M, V), -2 ** 30, np.int32)
    if kind == "alt":
        return (np.where((np.arange(M)[:, None] + np.arange(V)[None, :]) % 2 == 0, 2 ** 30, -2 ** 30)).astype(np.int32)
    if kind == "zero":
        return np.zeros((M, V), np.int32)
    assert kind == "random"          # vector 0 anywhere in +-2^30; the others small enough that h <= rec^2 / M <= rec: v >= 0
    v = np.zeros((M, V), np.int64)
    v[:, 0] = rng.integers(-2 ** 30, 2 ** 30 + 1, M)
    if V > 1:
        c = int(2 ** 30 / math.sqrt(M * (V - 1)))
        v[:, 1:] = rng.integers(-c, c + 1, (M, V - 1))
    return v.astype(np.int32)


def special_body(kind, seed, n_rows, N, kw, mode):
    """'zero': all-zero rows; 'ones': every column held, every padding bit set, counts 1; 'max': counts of 2^32 - 1 where held (about
    half the columns), PA as a half-full body"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (n_rows, 8 * kw), dtype=np.uint8)
    if kind == "zero":
        held = np.zeros((n_rows, N), bool)
    elif kind == "ones":
        held = np.ones((n_rows, N), bool)
    else:
        assert kind == "max"
        held = rng.random((n_rows, N)) < 0.5
    if mode == MODE_COUNT:
        c = np.where(held, U32 if kind == "max" else 1, 0).astype(np.uint32)
        if kind == "max":            # the unheld columns hold 1: below a = 2 and a = 2^32 - 1, at a = 1
            c[~held] = 1
        pay = c.astype("<u4").view(np.uint8).reshape(n_rows, 4 * N)
    else:
        bits = np.concatenate([held, np.ones((n_rows, (-N) % 8), bool)], axis=1)
        pay = np.packbits(bits, axis=1, bitorder="little").reshape(n_rows, (N + 7) // 8)
    return np.ascontiguousarray(np.concatenate([keys, pay], axis=1)).reshape(-1)


class Case:
    """One call.  thr: a number, or 'median' (the median of the statistics of the rows inside the window); vmin: a number, or 'above'
    (above every v: M + 1)"""

    def __init__(self, name, mode, n_cols, key_words, n_rows, cols, abund, vecs, frac_bits, gain, vmin, thr, min_rec, max_rec, make):
        self.name, self.mode, self.n_cols, self.key_words, self.n_rows, self.cols, self.abund = name, mode, n_cols, key_words, n_rows, cols, abund
        self.vecs, self.frac_bits, self.gain, self.min_rec, self.max_rec, self._make = vecs, frac_bits, gain, min_rec, max_rec, make
        self.n_use = n_cols if cols is None else len(cols)
        self.n_vec = vecs.shape[1]
        self.vmin = float(self.n_use + 1) if vmin == "above" else float(vmin)
        self._thr = thr

    @functools.cached_property
    def body(self):
        b = self._make()
        assert len(b) == self.n_rows * row_bytes(self.key_words, self.n_cols, self.mode)
        b.setflags(write=False)
        return b

    @functools.cached_property
    def all_rows(self):
        """the numpy road's word on every row, worked out once"""
        r = assoc_rows_np(self.body, self.n_cols, self.key_words, self.mode, self.vecs, self.frac_bits, self.gain, self.vmin, self.cols, self.abund)
        r.setflags(write=False)
        return r

    @functools.cached_property
    def threshold(self):
        if self._thr != "median":
            return float(self._thr)
        a = self.all_rows
        inside = a["stat"][(a["rec"] >= self.min_rec) & (a["rec"] <= self.max_rec)]
        return float(np.sort(inside)[len(inside) // 2]) if len(inside) else 0.0      # (an element: rows sit exactly on the threshold)

    @functools.cached_property
    def expected(self):
        """(the kept rows' records, the kept rows' bytes)"""
        a = self.all_rows
        keep = (a["rec"] >= self.min_rec) & (a["rec"] <= self.max_rec) & (a["stat"] >= self.threshold)
        rb = row_bytes(self.key_words, self.n_cols, self.mode)
        return a[keep], np.frombuffer(as_bytes(self.body), np.uint8).reshape(-1, rb)[keep].tobytes()

    def params(self):
        """the keyword arguments of Context.assoc / assoc_dev behind the body's"""
        return dict(vecs=self.vecs, frac_bits=self.frac_bits, gain=self.gain, vmin=self.vmin, threshold=self.threshold, cols=self.cols,
                    min_abund=self.abund, min_rec=self.min_rec, max_rec=self.max_rec)


COLUMNS = [1, 7, 63, 64, 65, 130, 513]                  # a byte, a block of 64 counts, a block of 64 payload bytes (512 columns) and past it
ROWS = [1, 63, 64, 65, 255, 256, 257, 700, 3000]        # both sides of a wave's group, of a placement tile; several tiles
VECTORS = [1, 2, 3, 17, 32]
V_CUTS = [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32]      # both sides of every step of VP_STEPS
SHAPES = ["uniform", 0.5, "skewed", "same"]
KINDS = ["none", "subset", "one", "second"]
VKINDS = ["random", "pos", "neg", "alt", "zero"]
THRS = [0.0, "median", INF]
ABUNDS = [1, 2, U32]


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """combinations, not the full product: every N in both modes and every value of the other axes -- they rotate at strides that are
    coprime to each other (test_assoc_cpu asserts the coverage)"""
    cases = []

    def add(name, mode, N, kw, rows, cols, a, vkind, V, vmin, thr, lo, hi, make, gain=3.7):
        M = N if cols is None else len(cols)
        cases.append(Case(name, mode, N, kw, rows, cols, a, make_vecs(vkind, M, V, 91 + len(cases)), 30, gain, vmin, thr, lo, hi, make))

    def window(i, M):
        return [(0, U32), (1, max(1, M - 1)), (M // 2 + 1, M // 2), (0, M // 2)][i % 4]      # the third is empty

    i = 0
    for N in COLUMNS:
        for mode in (MODE_COUNT, MODE_PA):
            for rep in range(3):
                rows = ROWS[(i * 3 + rep) % len(ROWS)]
                V = VECTORS[(i + 2 * rep) % len(VECTORS)]
                if rows * N * V > 3_000_000:      # (the long bodies ride on narrower matrices or fewer vectors: the Python road walks them)
                    rows = 700 if 700 * N * V <= 3_000_000 else 257
                kw = 1 + (i // 2 + i + rep) % 4
                shape = SHAPES[(i + rep) % len(SHAPES)]
                kind = KINDS[(i + rep) % len(KINDS)]
                vkind = VKINDS[(i * 2 + rep) % len(VKINDS)]
                thr = THRS[(i + rep) % len(THRS)]
                sd = 9000 + 10 * i + rep
                cols = make_cols(kind, N, sd)
                M = N if cols is None else len(cols)
                a = ABUNDS[(i + rep) % 3] if mode == MODE_COUNT else 1
                lo, hi = window(i + rep, M)
                vmin = [2.0 ** -10, 0.0, "above"][(i + rep) % 5 % 3]
                make = (lambda sd=sd, rows=rows, N=N, kw=kw, mode=mode, shape=shape: shaped_body(sd, rows, N, kw, mode, shape))
                m = "c" if mode == MODE_COUNT else "p"
                add(f"{m}-{N}-{kind}-r{rows}-k{kw}-{shape}-{vkind}{V}-a{a}-w{lo}_{hi}-t{thr}-v{vmin}", mode, N, kw, rows, cols, a, vkind, V, vmin, thr, lo, hi, make)
            i += 1
    # both sides of every step of the kernel's vector count, in both modes, the list a permuted subset so that unlisted columns are held
    for mode in (MODE_COUNT, MODE_PA):
        for n, V in enumerate(V_CUTS):
            sd = 9500 + n
            N = (65, 130)[n % 2] if mode == MODE_COUNT else (65, 520)[n % 2]
            cols = make_cols("subset", N, sd)
            make = (lambda sd=sd, N=N, mode=mode, n=n: shaped_body(sd, 130, N, 1 + n % 4, mode, "uniform"))
            add(f"{'c' if mode == MODE_COUNT else 'p'}-{N}-subset-r130-k{1 + n % 4}-uniform-random{V}-cut", mode, N, 1 + n % 4, 130, cols, 1, "random", V, 2.0 ** -10, "median", 1, len(cols) - 1, make)
    # PA: exactly one block of 64 payload bytes, and one byte more (COUNT: N = 64 / 65 above)
    for N in (512, 513):
        make = (lambda N=N: shaped_body(9600 + N, 257, N, 3, MODE_PA, "uniform"))
        add(f"p-{N}-none-r257-k3-uniform-random3-block", MODE_PA, N, 3, 257, None, 1, "random", 3, 0.0, "median", 0, U32, make)
    # the largest entries on every present column: every 32-bit partial sum wraps
    for mode in (MODE_COUNT, MODE_PA):
        for vkind in ("pos", "neg", "alt"):
            make = (lambda mode=mode: special_body("ones", 9700, 65, 130, 2, mode))
            add(f"{'c' if mode == MODE_COUNT else 'p'}-130-none-r65-k2-ones-{vkind}2-wrap", mode, 130, 2, 65, None, 1, vkind, 2, 0.0, 0.0, 0, U32, make)
    # the bodies at the edges: all-zero rows; every column and every padding bit set; counts of 2^32 - 1 at every min_abund
    for mode in (MODE_COUNT, MODE_PA):
        m = "c" if mode == MODE_COUNT else "p"
        for kind in ("zero", "ones"):
            make = (lambda mode=mode, kind=kind: special_body(kind, 9800, 257, 63, 1, mode))
            add(f"{m}-63-second-r257-k1-{kind}-random3-edge", mode, 63, 1, 257, make_cols("second", 63, 0), 1, "random", 3, 0.0, 0.0, 0, U32, make)
    for a in ABUNDS:
        make = (lambda: special_body("max", 9900, 255, 65, 4, MODE_COUNT))
        add(f"c-65-subset-r255-k4-max-random2-a{a}-edge", MODE_COUNT, 65, 4, 255, make_cols("subset", 65, 9900), a, "random", 2, 2.0 ** -10, "median", 1, 64, make)
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
