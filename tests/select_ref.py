"""The definition of `kmx select` (include/kmx.h, section "select") restated for the tests, by two roads that share no code: numpy over
whole columns (select_expected_np) and plain Python a row and a bit at a time (select_expected_py).  Beside them the list of bodies and
parameters that tests/test_select_gpu.py sends to the device: tests/test_select_cpu.py walks the same list, asserts that the two roads
agree on it and that its keep sets are not trivial."""
import functools
import struct
import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload, make_body, write_run, read_run_bodies  # noqa: F401

SELECT_REC = np.dtype([("row", "<u4"), ("rec", "<u4")])
U32 = 0xFFFFFFFF


def out_row_bytes(key_words, n_out, out_mode):
    return row_bytes(key_words, n_out, out_mode)


# ---- road 1: numpy over whole columns ---------------------------------------------------------------------------------------------
def select_expected_np(body, n_cols, key_words, mode, cols=None, out_mode=None, min_abund=1, min_rec=0, max_rec=None, zero_below=False):
    """-> (the kept rows at their new size as bytes, SELECT_REC array)"""
    out_mode = mode if out_mode is None else out_mode
    cols = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    M = len(cols)
    rb = row_bytes(key_words, n_cols, mode)
    raw = np.frombuffer(as_bytes(body), np.uint8).reshape(-1, rb)
    pay = split_payload(body, n_cols, key_words, mode)[:, cols]
    present = pay >= min_abund if mode == MODE_COUNT else pay
    rec = present.sum(axis=1).astype(np.int64)
    hi = M if max_rec is None or max_rec >= M else max_rec
    kept = np.flatnonzero((rec >= min_rec) & (rec <= hi))
    recs = np.zeros(len(kept), SELECT_REC)
    recs["row"], recs["rec"] = kept, rec[kept]
    keys = raw[kept, :8 * key_words]
    if out_mode == MODE_COUNT:
        v = pay[kept].astype("<u4")
        if zero_below:
            v = np.where(v < min_abund, 0, v).astype("<u4")
        new = np.ascontiguousarray(v).view(np.uint8).reshape(len(kept), 4 * M)
    else:
        new = np.packbits(present[kept], axis=1, bitorder="little").reshape(len(kept), (M + 7) // 8)
    return np.concatenate([keys, new], axis=1).tobytes(), recs


# ---- road 2: Python integers, a row and a bit at a time ---------------------------------------------------------------------------
def rows_py(body, n_cols, key_words, mode, cols, min_abund):
    """-> one (key bytes, values, present) a row: the selected columns' counts (PA: bits) and whether the sample holds the row"""
    raw, rb = as_bytes(body), row_bytes(key_words, n_cols, mode)
    assert len(raw) % rb == 0
    cols = list(range(n_cols)) if cols is None else [int(c) for c in cols]
    out = []
    for r in range(len(raw) // rb):
        row = raw[r * rb:(r + 1) * rb]
        pay = row[8 * key_words:]
        vals = []
        for c in cols:
            if mode == MODE_COUNT:
                vals.append(struct.unpack_from("<I", pay, 4 * c)[0])
            else:
                vals.append((pay[c >> 3] >> (c & 7)) & 1)
        present = [1 if v >= min_abund else 0 for v in vals] if mode == MODE_COUNT else vals
        out.append((row[:8 * key_words], vals, present))
    return out


def assemble_py(rows, mode, out_mode, min_abund, min_rec, max_rec, zero_below):
    """rows_py's rows -> (body bytes, [(row, rec)])"""
    body, recs = bytearray(), []
    for r, (key, vals, present) in enumerate(rows):
        M = len(vals)
        rec = sum(present)
        if rec < min_rec or (max_rec is not None and max_rec < M and rec > max_rec):
            continue
        recs.append((r, rec))
        body += key
        if out_mode == MODE_COUNT:
            assert mode == MODE_COUNT
            for v in vals:
                body += struct.pack("<I", 0 if zero_below and v < min_abund else v)
        else:
            bits = 0
            for j, p in enumerate(present):
                bits |= p << j
            body += bits.to_bytes((M + 7) // 8, "little")
    return bytes(body), recs


def select_expected_py(body, n_cols, key_words, mode, cols=None, out_mode=None, min_abund=1, min_rec=0, max_rec=None, zero_below=False):
    out_mode = mode if out_mode is None else out_mode
    return assemble_py(rows_py(body, n_cols, key_words, mode, cols, min_abund), mode, out_mode, min_abund, min_rec, max_rec, zero_below)


# ---- what the GPU test sends: one list, walked by both test files --------------------------------------------------------------------
def make_cols(kind, N, M, seed):
    """the column lists of the sweep -> a uint32 array, or None (the identity said by leaving the list out)"""
    if kind == "none":
        return None
    if kind == "identity":
        return np.arange(N, dtype=np.uint32)
    if kind == "reversed":
        return np.arange(N, dtype=np.uint32)[::-1].copy()
    if kind == "every-other":
        return np.arange(0, N, 2, dtype=np.uint32)
    if kind == "one":
        return np.array([N // 2], np.uint32)
    assert kind == "perm"
    return np.random.default_rng(seed).permutation(N)[:M].astype(np.uint32)


def rec_ranges(M):
    """(min_rec, max_rec): all, held by one at least, held by all, one to all but one, none"""
    return [(0, M), (1, M), (M, M), (1, M - 1), (2, 1)]


class Case:
    """a body, a column list, and the parameter sets it is run with: dicts of min_abund, min_rec, max_rec, out_mode, zero_below"""

    def __init__(self, name, mode, out_mode, n_cols, key_words, n_rows, cols, runs, make):
        self.name, self.mode, self.out_mode, self.n_cols, self.key_words, self.n_rows = name, mode, out_mode, n_cols, key_words, n_rows
        self.cols, self.runs, self._make = cols, runs, make
        self.n_out = n_cols if cols is None else len(cols)

    @functools.cached_property
    def body(self):
        b = self._make()
        assert len(b) == self.n_rows * row_bytes(self.key_words, self.n_cols, self.mode)
        b.setflags(write=False)
        return b

    @functools.cached_property
    def expected(self):
        """the numpy road's word on every run, worked out once: [(body bytes, recs)]"""
        return [select_expected_np(self.body, self.n_cols, self.key_words, self.mode, self.cols, **r) for r in self.runs]


# (N, kind of list, M): every N and every M of the sweep, both sides of a byte and of a wave's worth of units, lists left out and given
COLUMN_SHAPES = [(1, "identity", 1), (7, "reversed", 7), (8, "perm", 7), (8, "every-other", 4), (9, "perm", 8), (9, "one", 1),
                 (63, "perm", 9), (63, "none", 63), (64, "reversed", 64), (64, "none", 64), (65, "perm", 63), (65, "identity", 65),
                 (130, "perm", 64), (130, "every-other", 65), (520, "perm", 65), (520, "every-other", 260), (520, "none", 520),
                 (520, "one", 1)]
WIDE_COUNT_SHAPES = [(2049, "every-other", 1025), (2049, "perm", 1000), (2100, "every-other", 1050), (2100, "perm", 1000)]
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 4200]
FILLS = [0.0, 0.02, 0.5, 1.0]
ABUNDS = [1, 2, U32]
MODE_PAIRS = [(MODE_COUNT, MODE_COUNT), (MODE_COUNT, MODE_PA), (MODE_PA, MODE_PA)]
PAIR_NAMES = {(MODE_COUNT, MODE_COUNT): "cc", (MODE_COUNT, MODE_PA): "cp", (MODE_PA, MODE_PA): "pp"}


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """combinations, not the full product: every pair of (column shape, mode pair) appears, and every value of the other axes does --
    they rotate at strides that are coprime to each other (test_select_cpu asserts the coverage)"""
    cases = []
    i = 0
    for si, (N, kind, M) in enumerate(COLUMN_SHAPES):
        for pi, (mode, out_mode) in enumerate(MODE_PAIRS):
            rows = ROWS[(i * 2 + si) % len(ROWS)]
            kw = 1 + (i + pi) % 4
            fill = FILLS[(i + si // 4) % len(FILLS)]
            if rows == 4200 and N == 520 and mode == MODE_COUNT:
                rows = 257      # (the long bodies ride on narrower matrices: a few hundred KB each)
            sd = 7000 + i
            cols = make_cols(kind, N, M, sd)
            m = N if cols is None else len(cols)
            assert m == M
            runs = []
            for ri, (lo, hi) in enumerate(rec_ranges(M)):
                a = ABUNDS[(i + ri) % 3] if mode == MODE_COUNT else 1
                zb = out_mode == MODE_COUNT and (i + ri) % 2 == 1
                runs.append(dict(out_mode=out_mode, min_abund=a, min_rec=lo, max_rec=hi, zero_below=zb))
            make = (lambda sd=sd, rows=rows, N=N, kw=kw, mode=mode, fill=fill:
                    make_body(sd, rows, N, kw, mode, fill=fill, pad_ones=True, maxed=0.05, lo=1, hi=4))
            cases.append(Case(f"{PAIR_NAMES[(mode, out_mode)]}-{N}-{kind}-{M}-r{rows}-k{kw}-f{fill}", mode, out_mode, N, kw, rows, cols, runs, make))
            i += 1
    # proper subsets by design: a = 2 on counts 1 ... 3 at fill 0.5 over 8 of 9 columns, rec within 2 ... 3; several placement tiles
    for mode, out_mode in MODE_PAIRS:
        sd = 7900 + len(cases)
        a = 2 if mode == MODE_COUNT else 1
        runs = [dict(out_mode=out_mode, min_abund=a, min_rec=2, max_rec=3, zero_below=out_mode == MODE_COUNT),
                dict(out_mode=out_mode, min_abund=a, min_rec=3, max_rec=None, zero_below=False)]
        make = (lambda sd=sd, mode=mode: make_body(sd, 1000, 9, 2, mode, fill=0.5, pad_ones=True, maxed=0.05, lo=1, hi=4))
        cases.append(Case(f"{PAIR_NAMES[(mode, out_mode)]}-subset", mode, out_mode, 9, 2, 1000, make_cols("perm", 9, 8, sd), runs, make))
    # (appended behind the cases above: the running index goes on, no earlier seed moves)
    # count columns on both sides of the 32 units a lane of k_select_score keeps the selection of in a register (64 lanes x 32 = 2048
    # columns): beyond them it comes from memory; the lists take some of the columns out there and leave some
    for N, kind, M in WIDE_COUNT_SHAPES:
        for mode, out_mode in MODE_PAIRS[:2]:
            rows, kw, fill = 150, 1 + i % 4, 0.5
            sd = 7000 + i
            cols = make_cols(kind, 2048 if (N, kind) == (2049, "perm") else N, M, sd)      # (N = 2049: "perm" leaves the one column out there)
            assert len(cols) == M
            runs = []
            for ri, (lo, hi) in enumerate(rec_ranges(M)[:4]):
                a = ABUNDS[(i + ri) % 2]
                runs.append(dict(out_mode=out_mode, min_abund=a, min_rec=lo, max_rec=hi, zero_below=out_mode == MODE_COUNT and (i + ri) % 2 == 1))
            # (half the selected columns hold a row on average: about half the rows are kept)
            runs.append(dict(out_mode=out_mode, min_abund=1, min_rec=M // 2, max_rec=M, zero_below=False))
            make = (lambda sd=sd, rows=rows, N=N, kw=kw, fill=fill: make_body(sd, rows, N, kw, MODE_COUNT, fill=fill, pad_ones=True, maxed=0.05, lo=1, hi=4))
            cases.append(Case(f"{PAIR_NAMES[(mode, out_mode)]}-{N}-{kind}-{M}-r{rows}-k{kw}-f{fill}", mode, out_mode, N, kw, rows, cols, runs, make))
            i += 1
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
