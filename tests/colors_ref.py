"""The definition of `kmx colors` (include/kmx.h, section "colors") restated for the tests, by two roads that share no code: plain
Python integers a row and a bit at a time, the classes in a dict whose insertion order IS the class order (colors_expected_py), and
numpy -- the packed rows through np.unique, reordered by first index (colors_expected_np).  Beside them the identities of the header,
the driver's table and --ids files restated, and the list of bodies and parameters that tests/test_colors_gpu.py sends to the device."""
import functools
import struct

import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload, make_body, write_run, read_run_bodies  # noqa: F401
from pan_ref import make_cols, pan_expected_np  # noqa: F401

U32 = 0xFFFFFFFF


class Classes:
    """n_classes C; ids [n_rows]; first [C]; sizes [C]; patterns [C][W] -- lists of Python integers"""

    def __init__(self, ids, first, sizes, patterns, W):
        self.n_classes, self.ids, self.first, self.sizes, self.patterns, self.W = len(first), ids, first, sizes, patterns, W

    def as_lists(self):
        return self.n_classes, self.ids, self.first, self.sizes, self.patterns


# ---- road 1: Python integers, a row and a bit at a time ---------------------------------------------------------------------------
def colors_expected_py(body, n_cols, key_words, mode, cols=None, min_abund=1):
    raw, rb, N = as_bytes(body), row_bytes(key_words, n_cols, mode), n_cols
    assert len(raw) % rb == 0
    cols = list(range(N)) if cols is None else [int(c) for c in cols]
    M = len(cols)
    W = (M + 63) // 64
    seen = {}      # pattern (one integer of M bits) -> class, in the order of the first rows
    ids, first, sizes = [], [], []
    for r in range(len(raw) // rb):
        pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
        p = 0
        for j, c in enumerate(cols):
            if mode == MODE_COUNT:
                present = struct.unpack_from("<I", pay, 4 * c)[0] >= min_abund
            else:
                present = bool((pay[c >> 3] >> (c & 7)) & 1)
            p |= int(present) << j
        if p not in seen:
            seen[p] = len(first)
            first.append(r); sizes.append(0)
        ids.append(seen[p])
        sizes[seen[p]] += 1
    patterns = [[(p >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(W)] for p in seen]
    return Classes(ids, first, sizes, patterns, W)


# ---- road 2: numpy, np.unique over the packed rows --------------------------------------------------------------------------------
def colors_expected_np(body, n_cols, key_words, mode, cols=None, min_abund=1):
    """-> (C, ids uint32 [rows], first uint32 [C], sizes uint32 [C], patterns uint64 [C, W])"""
    cols = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    M = len(cols)
    W = (M + 63) // 64
    pay = split_payload(body, n_cols, key_words, mode)[:, cols]
    present = pay >= min_abund if mode == MODE_COUNT else pay.astype(bool)
    n = len(present)
    padded = np.concatenate([present, np.zeros((n, 64 * W - M), bool)], axis=1)
    packed = np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(n, W)
    if n == 0:
        return 0, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, W), np.uint64)
    uniq, first, inverse, counts = np.unique(packed, axis=0, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")      # np.unique sorts by value: the classes are wanted in the order of their first rows
    new_id = np.empty(len(order), np.int64)
    new_id[order] = np.arange(len(order))
    return (len(order), new_id[np.asarray(inverse).reshape(-1)].astype(np.uint32), first[order].astype(np.uint32), counts[order].astype(np.uint32),
            np.ascontiguousarray(uniq[order]).astype(np.uint64))


def popcounts(patterns):
    return [sum(bin(int(w)).count("1") for w in p) for p in patterns]


def check_identities(n_classes, ids, first, sizes, patterns, n_rows, M, row_pattern=None, spectrum0=None):
    """the identities of the header; row_pattern(r) -> the W words of row r, worked out elsewhere; spectrum0: kmx_pan's spectrum[0]"""
    ids, first, sizes = [int(x) for x in ids], [int(x) for x in first], [int(x) for x in sizes]
    assert len(ids) == n_rows and len(first) == len(sizes) == len(patterns) == n_classes
    assert sum(sizes) == n_rows
    assert all(ids[first[c]] == c for c in range(n_classes))
    assert all(first[c] < first[c + 1] for c in range(n_classes - 1))
    assert all(0 <= i < n_classes for i in ids)
    assert len({tuple(int(w) for w in p) for p in patterns}) == n_classes      # no class twice
    if M % 64 and n_classes:
        assert all(int(p[-1]) >> (M % 64) == 0 for p in patterns)              # unused high bits are zero
    if row_pattern is not None:
        for c in range(n_classes):
            assert [int(w) for w in row_pattern(first[c])] == [int(w) for w in patterns[c]], c
    if spectrum0 is not None:
        by_rec = [0] * (M + 1)
        for s, k in zip(sizes, popcounts(patterns)):
            by_rec[k] += s
        assert by_rec == [int(x) for x in spectrum0]


# ---- the driver's texts -----------------------------------------------------------------------------------------------------------
def bits_text(pattern, M):
    return "".join("1" if (int(pattern[j >> 6]) >> (j & 63)) & 1 else "0" for j in range(M))


def sorted_table(table, M):
    """table: {pattern tuple: rows} -> [(pattern, rows)] rows descending, ties by the 0/1 string ascending"""
    return sorted(table.items(), key=lambda kv: (-kv[1], bits_text(kv[0], M)))


def colors_text(ids, min_abund, table, top=None):
    """the text `kmx colors` prints for the merged class table {pattern tuple of W words: rows}"""
    M = len(ids)
    rows = sorted_table(table, M)
    shown = len(rows) if top is None else min(top, len(rows))
    lines = ["# kmx colors", f"# samples: {M}", f"# rows: {sum(table.values())}", f"# classes: {len(rows)}", f"# min_abund: {min_abund}", f"# shown: {shown}",
             "rank\trows\trec\tpattern\tsamples"]
    for k, (p, n) in enumerate(rows[:shown]):
        bits = bits_text(p, M)
        held = [ids[j] for j in range(M) if bits[j] == "1"]
        lines.append(f"{k}\t{n}\t{len(held)}\t{bits}\t{','.join(held) if held else '-'}")
    return "\n".join(lines) + "\n"


def merged_table(parts):
    """parts: colors_expected_np results, one a partition -> ({pattern tuple: rows}, per partition the pattern tuple of every row)"""
    table, row_patterns = {}, []
    for C, ids, first, sizes, patterns in parts:
        pats = [tuple(int(w) for w in p) for p in patterns]
        for p, s in zip(pats, sizes):
            table[p] = table.get(p, 0) + int(s)
        row_patterns.append([pats[i] for i in ids])
    return table, row_patterns


def ids_files(table, row_patterns, M):
    """--ids: per partition the little-endian u32 rank of every row's class in the full sorted table"""
    rank = {p: k for k, (p, _) in enumerate(sorted_table(table, M))}
    return [np.array([rank[p] for p in rows], "<u4").tobytes() for rows in row_patterns]


def parse_colors(text):
    """the text `kmx colors` prints -> (dict of the comment lines, [(rank, rows, rec, bits, samples)])"""
    lines = text.splitlines()
    assert lines[0] == "# kmx colors"
    head, i = {}, 1
    while lines[i].startswith("# "):
        k, v = lines[i][2:].split(": ", 1)
        head[k] = v
        i += 1
    assert list(head) == ["samples", "rows", "classes", "min_abund", "shown"]
    assert lines[i] == "rank\trows\trec\tpattern\tsamples"
    rows = []
    for ln in lines[i + 1:]:
        c = ln.split("\t")
        assert len(c) == 5
        rows.append((int(c[0]), int(c[1]), int(c[2]), c[3], c[4]))
    assert len(rows) == int(head["shown"])
    return head, rows


# ---- what the GPU test sends ------------------------------------------------------------------------------------------------------
def structured_body(seed, n_rows, N, kw, mode, structure, cols=None):
    """class structures: 'one' every row equal; 'distinct' every row its own pattern where 2^M allows (else as many as there are);
    'skewed' 60 % one class, 30 % a second, singletons after; 'alternate' two classes row by row; 'last' patterns that differ only in
    the LAST listed column; 'random' every column present with probability 1/2.  PA: every padding bit set.  Counts are 1 ... 3, a
    twentieth of the present ones 2^32 - 1."""
    rng = np.random.default_rng(seed)
    listed = np.arange(N) if cols is None else np.asarray(cols, np.int64)
    M = len(listed)
    held = np.zeros((n_rows, N), bool)
    base = rng.random(N) < 0.5
    if structure == "one":
        held[:] = base
    elif structure == "alternate":
        other = base.copy(); other[listed[0]] ^= True
        held[0::2] = base; held[1::2] = other
    elif structure == "last":
        held[:] = base
        held[:, listed[-1]] = rng.random(n_rows) < 0.5
    elif structure == "random":
        held = rng.random((n_rows, N)) < 0.5
    else:
        # row r's pattern over the list is the binary number r (distinct), folded where M bits do not hold n_rows numbers
        numbers = np.arange(n_rows, dtype=np.uint64) % np.uint64(2 ** min(M, 40))
        bits = ((numbers[:, None] >> np.arange(min(M, 40), dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        held[:] = base
        held[:, listed[:bits.shape[1]]] = bits
        if structure == "skewed":
            share = rng.random(n_rows)
            a, b = base.copy(), base.copy()
            a[listed] = True; b[listed] = False
            held[share < 0.6] = a
            held[(share >= 0.6) & (share < 0.9)] = b
        else:
            assert structure == "distinct"
    keys = rng.integers(0, 256, (n_rows, 8 * kw), dtype=np.uint8)
    if mode == MODE_COUNT:
        c = rng.integers(1, 4, (n_rows, N)).astype(np.uint32)
        c[rng.random((n_rows, N)) < 0.05] = U32
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
        """the numpy road's word for every min_abund of the case, worked out once: {a: (C, ids, first, sizes, patterns)}"""
        return {a: colors_expected_np(self.body, self.n_cols, self.key_words, self.mode, self.cols, a) for a in self.abunds}


COLUMNS = [1, 7, 8, 9, 63, 64, 65, 130, 257, 1025]
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 700, 4200]
STRUCTURES = ["one", "distinct", "skewed", "alternate", "last", "random"]
KINDS = ["none", "reversed", "scattered", "one"]
ABUNDS = [1, 2, U32]


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """combinations, not the full product: every N in both modes, and every value of the other axes -- they rotate at strides that are
    coprime to each other (test_colors_cpu asserts the coverage)"""
    cases = []
    i = 0
    for N in COLUMNS:
        for mode in (MODE_COUNT, MODE_PA):
            for rep in range(3):
                q = i // 6 * 3 + rep      # the case's number inside its mode
                rows = ROWS[q % len(ROWS)]
                if mode == MODE_COUNT and N >= 1000 and rows > 700:
                    rows = 700      # (the long bodies ride on narrower matrices: a few MB at the most)
                kw = 1 + (q + q // 10) % 4
                structure = STRUCTURES[(q + q // 6) % len(STRUCTURES)]
                kind = KINDS[(q + q // 4) % len(KINDS)]
                sd = 21000 + i
                cols = make_cols(kind, N, sd)
                abunds = (ABUNDS[q % 3], ABUNDS[(q + 1) % 3]) if mode == MODE_COUNT else (1,)
                make = (lambda sd=sd, rows=rows, N=N, kw=kw, mode=mode, structure=structure, cols=cols: structured_body(sd, rows, N, kw, mode, structure, cols))
                m = "c" if mode == MODE_COUNT else "p"
                cases.append(Case(f"{m}-{N}-{kind}-r{rows}-k{kw}-{structure}", mode, N, kw, rows, cols, abunds, make))
                i += 1
    # the longest bodies in the structures that stress the table: one hot address, every row a class, the skew of a real matrix
    for mode in (MODE_COUNT, MODE_PA):
        for N, rows, structure, kind in ((9, 4200, "one", "none"), (65, 4200, "distinct", "reversed"), (130, 4200, "skewed", "scattered"), (64, 4200, "alternate", "none"),
                                         (257, 4200, "last", "scattered"), (40, 4200, "distinct", "none")):
            sd = 21500 + len(cases)
            cols = make_cols(kind, N, sd)
            make = (lambda sd=sd, rows=rows, N=N, mode=mode, structure=structure, cols=cols: structured_body(sd, rows, N, 1, mode, structure, cols))
            m = "c" if mode == MODE_COUNT else "p"
            cases.append(Case(f"{m}-{N}-{kind}-r{rows}-k1-{structure}-long", mode, N, 1, rows, cols, (1,), make))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
