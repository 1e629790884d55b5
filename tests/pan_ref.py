"""The definition of `kmx pan` (include/kmx.h, section "pan") restated for the tests, by two roads that share no code: plain Python
integers a row and a bit at a time (pan_expected_py) and numpy over whole columns (pan_expected_np).  Beside them the curves of the driver
in exact fractions.Fraction, the same curves by brute force over every order of adding the samples, the driver's texts, and the list of
bodies and parameters that tests/test_pan_gpu.py sends to the device."""
import functools
import itertools
import math
import struct
from fractions import Fraction

import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload, make_body, write_run, read_run_bodies  # noqa: F401

U32 = 0xFFFFFFFF


# ---- road 1: Python integers, a row and a bit at a time ---------------------------------------------------------------------------
def pan_expected_py(body, n_cols, key_words, mode, cols=None, min_abund=1):
    """-> (spectrum: three lists of M + 1 integers, shared: M + 1 lists of n_cols integers)"""
    raw, rb, N = as_bytes(body), row_bytes(key_words, n_cols, mode), n_cols
    assert len(raw) % rb == 0
    cols = list(range(N)) if cols is None else [int(c) for c in cols]
    M = len(cols)
    spec = [[0] * (M + 1) for _ in range(3)]
    shared = [[0] * N for _ in range(M + 1)]
    for r in range(len(raw) // rb):
        pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
        present = []
        for c in cols:
            if mode == MODE_COUNT:
                present.append(struct.unpack_from("<I", pay, 4 * c)[0] >= min_abund)
            else:
                present.append(bool((pay[c >> 3] >> (c & 7)) & 1))
        rec = sum(present)
        first = next((j for j in range(M) if present[j]), M)
        gap = next((j for j in range(M) if not present[j]), M)
        spec[0][rec] += 1; spec[1][first] += 1; spec[2][gap] += 1
        for j in range(M):
            if present[j]:
                shared[rec][cols[j]] += 1
    return spec, shared


# ---- road 2: numpy over whole columns ---------------------------------------------------------------------------------------------
def pan_expected_np(body, n_cols, key_words, mode, cols=None, min_abund=1):
    """-> (spectrum uint64 [3, M + 1], shared uint64 [M + 1, n_cols])"""
    cols = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    M = len(cols)
    pay = split_payload(body, n_cols, key_words, mode)[:, cols]
    present = pay >= min_abund if mode == MODE_COUNT else pay.astype(bool)
    rec = present.sum(axis=1).astype(np.int64)
    first = np.where(present.any(axis=1), present.argmax(axis=1), M)
    gap = np.where(present.all(axis=1), M, (~present).argmax(axis=1))
    spec = np.stack([np.bincount(x, minlength=M + 1) for x in (rec, first, gap)]).astype(np.uint64)
    in_list = np.zeros((M + 1, M), np.uint64)
    for r in np.unique(rec):
        in_list[r] = present[rec == r].sum(axis=0, dtype=np.uint64)
    shared = np.zeros((M + 1, n_cols), np.uint64)
    shared[:, cols] = in_list
    return spec, shared


def check_identities(spec, shared, n_rows, cols, n_cols, holders=None):
    """the five identities of the header on one call's increments (holders: the rows that hold input column c, from elsewhere)"""
    spec, shared = np.asarray(spec, np.uint64), np.asarray(shared, np.uint64)
    M = spec.shape[1] - 1
    assert int(spec[0].sum()) == int(spec[1].sum()) == int(spec[2].sum()) == n_rows
    assert spec[1][M] == spec[0][0] and spec[2][M] == spec[0][M]
    assert [int(x) for x in shared.sum(axis=1)] == [r * int(spec[0][r]) for r in range(M + 1)]
    listed = np.zeros(n_cols, bool)
    listed[np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)] = True
    assert not shared[:, ~listed].any() and not shared[0].any()
    if holders is not None:
        assert [int(x) for x in shared.sum(axis=0)] == [int(h) if l else 0 for h, l in zip(holders, listed)]


# ---- the curves, exact ------------------------------------------------------------------------------------------------------------
def curves_exact(spec):
    """spec [3][M + 1] of integers -> dict of lists indexed 1 ... M (entry 0 None): the means as Fractions, the ordered curves as ints"""
    h, first, gap = ([int(x) for x in row] for row in spec)
    M = len(h) - 1
    C = math.comb
    out = {k: [None] * (M + 1) for k in ("pan_mean", "core_mean", "new_mean", "pan_order", "core_order")}
    rs = [r for r in range(1, M + 1) if h[r]]
    for m in range(1, M + 1):      # (the terms of one m share a denominator: integer sums, one Fraction)
        cm, cp = C(M, m), C(M, m - 1) * (M - m + 1)
        out["pan_mean"][m] = Fraction(sum(h[r] * (cm - C(M - r, m)) for r in rs), cm)
        out["core_mean"][m] = Fraction(sum(h[r] * C(r, m) for r in rs if r >= m), cm)
        out["new_mean"][m] = Fraction(sum(h[r] * C(M - r, m - 1) * r for r in rs), cp)
        out["pan_order"][m] = sum(first[:m])
        out["core_order"][m] = sum(gap[m:])
    return out


def curves_brute(present):
    """present: bool [rows, M] in list order.  The averages over ALL M! orders, on the matrix itself -> (pan, core, new) lists of
    Fractions indexed 1 ... M; and (pan_order, core_order) in the order given"""
    present = np.asarray(present, bool)
    M = present.shape[1]
    tot = {k: [0] * (M + 1) for k in ("pan", "core", "new")}
    n = 0
    for perm in itertools.permutations(range(M)):
        n += 1
        seen = np.zeros(len(present), bool)
        core = np.ones(len(present), bool)
        for m, j in enumerate(perm, 1):
            before = int(seen.sum())
            seen |= present[:, j]
            core &= present[:, j]
            tot["pan"][m] += int(seen.sum()); tot["core"][m] += int(core.sum()); tot["new"][m] += int(seen.sum()) - before
    mean = {k: [None] + [Fraction(v, n) for v in vs[1:]] for k, vs in tot.items()}
    pan_o = [None] + [int(present[:, :m].any(axis=1).sum()) for m in range(1, M + 1)]
    core_o = [None] + [int(present[:, :m].all(axis=1).sum()) for m in range(1, M + 1)]
    return mean, pan_o, core_o


def heaps_alpha(new_mean):
    """minus the least-squares slope of ln new_mean(m) on ln m over the m in 2 ... M with new_mean(m) > 0; None below 3 points.
    new_mean: exact values indexed 1 ... M"""
    pts = [(math.log(m), math.log(Fraction(v).numerator) - math.log(Fraction(v).denominator)) for m, v in enumerate(new_mean) if m >= 2 and v is not None and v > 0]
    if len(pts) < 3:
        return None
    mx, my = math.fsum(x for x, _ in pts) / len(pts), math.fsum(y for _, y in pts) / len(pts)
    return -math.fsum((x - mx) * (y - my) for x, y in pts) / math.fsum((x - mx) ** 2 for x, _ in pts)


# ---- the driver's texts -----------------------------------------------------------------------------------------------------------
def spectrum_text(ids, min_abund, spec):
    M = len(ids)
    lines = ["# kmx pan spectrum", f"# samples: {M}", f"# min_abund: {min_abund}"] + [f"# id: {s}" for s in ids] + ["r\trows\tfirst\tgap"]
    lines += [f"{r}\t{int(spec[0][r])}\t{int(spec[1][r])}\t{int(spec[2][r])}" for r in range(M + 1)]
    return "\n".join(lines) + "\n"


def shared_text(ids, cols, shared):
    """the (M + 1) x M table in list order"""
    M = len(ids)
    cols = list(range(M)) if cols is None else [int(c) for c in cols]
    lines = ["r" + "".join("\t" + s for s in ids)]
    lines += ["\t".join([str(r)] + [str(int(shared[r][c])) for c in cols]) for r in range(M + 1)]
    return "\n".join(lines) + "\n"


def parse_curves(text):
    """the text `kmx pan` prints -> (dict of the comment lines, [(m, id, pan_mean, core_mean, new_mean, pan_order, core_order)] with
    the means as the strings printed)"""
    head, rows = {}, []
    lines = text.splitlines()
    assert lines[0] == "# kmx pan"
    i = 1
    while lines[i].startswith("# "):
        k, v = lines[i][2:].split(": ", 1)
        head[k] = v
        i += 1
    assert list(head) == ["samples", "rows", "min_abund", "heaps_alpha"]
    assert lines[i] == "m\tsample\tpan_mean\tcore_mean\tnew_mean\tpan_order\tcore_order"
    for ln in lines[i + 1:]:
        c = ln.split("\t")
        assert len(c) == 7 and all(re_fixed(x) for x in c[2:5])
        rows.append((int(c[0]), c[1], c[2], c[3], c[4], int(c[5]), int(c[6])))
    assert [r[0] for r in rows] == list(range(1, int(head["samples"]) + 1))
    return head, rows


def re_fixed(x):
    a, _, b = x.partition(".")
    return a.isdigit() and b.isdigit() and len(b) == 6


# ---- what the GPU test sends ------------------------------------------------------------------------------------------------------
def make_cols(kind, N, seed):
    """the lists of the sweep -> a uint32 array, or None (the identity said by leaving the list out)"""
    if kind == "none":
        return None
    if kind == "identity":
        return np.arange(N, dtype=np.uint32)
    if kind == "reversed":
        return np.arange(N, dtype=np.uint32)[::-1].copy()
    if kind == "one":
        return np.array([N // 2], np.uint32)
    assert kind == "scattered"
    return np.random.default_rng(seed).permutation(N)[:max(1, (2 * N) // 3)].astype(np.uint32)


def shaped_body(seed, n_rows, N, kw, mode, shape, maxed=0.05):
    """recurrence shapes: 'skewed' rows private or core only; 'uniform' every r about as often; 'same' every row the same r (N // 2,
    at least 1); 'zero' all-zero rows; a float: every column present with that probability.  PA: every padding bit set."""
    rng = np.random.default_rng(seed)
    if isinstance(shape, float):
        return make_body(seed, n_rows, N, kw, mode, fill=shape, pad_ones=True, maxed=maxed, lo=1, hi=4)
    if shape == "zero":
        held = np.zeros((n_rows, N), bool)
    elif shape == "skewed":
        held = np.zeros((n_rows, N), bool)
        core = rng.random(n_rows) < 0.4
        held[core] = True
        held[~core, rng.integers(0, N, int((~core).sum()))] = True
    else:
        k = np.full(n_rows, max(1, N // 2)) if shape == "same" else rng.integers(0, N + 1, n_rows)
        held = np.argsort(rng.random((n_rows, N)), axis=1) < k[:, None]
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


class Case:
    def __init__(self, name, mode, n_cols, key_words, n_rows, cols, abunds, make):
        self.name, self.mode, self.n_cols, self.key_words, self.n_rows, self.cols, self.abunds, self._make = name, mode, n_cols, key_words, n_rows, cols, abunds, make
        self.n_use = n_cols if cols is None else len(cols)

    @functools.cached_property
    def body(self):
        b = self._make()
        assert len(b) == self.n_rows * row_bytes(self.key_words, self.n_cols, self.mode)
        b.setflags(write=False)
        return b

    @functools.cached_property
    def expected(self):
        """the numpy road's word for every min_abund of the case, worked out once: {a: (spectrum, shared)}"""
        return {a: pan_expected_np(self.body, self.n_cols, self.key_words, self.mode, self.cols, a) for a in self.abunds}


LDS_MAX_M = 4095      # the largest M whose three histograms k_pan_score keeps in LDS (PN_LDS_WORDS = 12288 = 3 * 4096)
COLUMNS = [1, 7, 8, 9, 63, 64, 65, 130, 257, 520, 1000, 1025, 2100]
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 700, 4200, 12293]
SHAPES = ["skewed", "uniform", "same", "zero", 0.02, 0.5, 1.0]
KINDS = ["none", "identity", "reversed", "scattered", "one"]
ABUNDS = [1, 2, U32]


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """combinations, not the full product: every N in both modes, and every value of the other axes -- they rotate at strides that are
    coprime to each other (test_pan_cpu asserts the coverage)"""
    cases = []
    i = 0
    for N in COLUMNS:
        for mode in (MODE_COUNT, MODE_PA):
            for rep in range(2):
                rows = ROWS[(i * 3 + rep) % len(ROWS)]
                if mode == MODE_COUNT and N >= 1000 and rows > 700:
                    rows = 700 if N == 1000 else 257      # (the long bodies ride on narrower matrices: a few MB at the most)
                kw = 1 + (i // 2 + i) % 4
                shape = SHAPES[(i + rep * 3) % len(SHAPES)]
                kind = KINDS[i % len(KINDS)]
                sd = 9000 + i
                cols = make_cols(kind, N, sd)
                abunds = (ABUNDS[i % 3], ABUNDS[(i + 1) % 3]) if mode == MODE_COUNT else (1,)
                make = (lambda sd=sd, rows=rows, N=N, kw=kw, mode=mode, shape=shape: shaped_body(sd, rows, N, kw, mode, shape))
                m = "c" if mode == MODE_COUNT else "p"
                cases.append(Case(f"{m}-{N}-{kind}-r{rows}-k{kw}-{shape}", mode, N, kw, rows, cols, abunds, make))
                i += 1
    # the longest bodies on narrow matrices, in the shapes that stress the order: one hot class, every class, two classes
    for mode in (MODE_COUNT, MODE_PA):
        for N, rows, shape, kind in ((9, 12293, "same", "none"), (65, 12293, "uniform", "reversed"), (130, 4200, "skewed", "scattered"), (64, 4200, "uniform", "none")):
            sd = 9500 + len(cases)
            make = (lambda sd=sd, rows=rows, N=N, mode=mode, shape=shape: shaped_body(sd, rows, N, 1, mode, shape))
            m = "c" if mode == MODE_COUNT else "p"
            cases.append(Case(f"{m}-{N}-{kind}-r{rows}-k1-{shape}-long", mode, N, 1, rows, make_cols(kind, N, sd), (1,), make))
    # both sides of the M that ends the LDS histograms; lists that take and that leave the far columns
    for mode in (MODE_COUNT, MODE_PA):
        for N, kind in ((LDS_MAX_M, "none"), (LDS_MAX_M + 1, "none"), (LDS_MAX_M + 1, "reversed"), (LDS_MAX_M + 6, "lds"), (LDS_MAX_M + 6, "scattered")):
            sd = 9700 + len(cases)
            rows = 70 if mode == MODE_COUNT else 300
            cols = np.random.default_rng(sd).permutation(N)[:LDS_MAX_M].astype(np.uint32) if kind == "lds" else make_cols(kind, N, sd)
            make = (lambda sd=sd, rows=rows, N=N, mode=mode: shaped_body(sd, rows, N, 2, mode, "uniform"))
            m = "c" if mode == MODE_COUNT else "p"
            cases.append(Case(f"{m}-{N}-{kind}-r{rows}-k2-uniform-edge", mode, N, 2, rows, cols, (1,), make))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
