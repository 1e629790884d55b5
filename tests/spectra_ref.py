"""The definition of `kmx spectra` (include/kmx.h, section "spectra") restated for the tests, by two roads that share no code: plain
Python integers a row at a time (spectra_expected_py) and numpy over whole columns with np.minimum and np.bincount
(spectra_expected_np).  Beside them the launcher's plan of the pairs restated (for algo_bytes), the driver's statistics in exact
fractions.Fraction, the driver's texts, and the list of bodies and parameters that tests/test_spectra_gpu.py sends to the device."""
import functools
import math
import struct
from fractions import Fraction

import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload, write_run, read_run_bodies  # noqa: F401

U32 = 0xFFFFFFFF
HIST_LDS_CAP = 255        # spectra.hip SP_HIST_LDS_CAP: the largest C1 whose bins live in LDS
JOINT_LDS_CAP = 109       # SP_JOINT_LDS_CAP: the largest C2 whose tables live in LDS
JOINT_LDS_WORDS = 12288   # SP_JOINT_LDS_WORDS
GROUP = 16                # SP_GROUP


# ---- road 1: Python integers, a row at a time -------------------------------------------------------------------------------------
def spectra_expected_py(body, n_cols, key_words, mode, cols=None, cap=255, pairs=None, joint_cap=63):
    """-> (hist: M lists of cap + 2 integers, joint: P lists of joint_cap + 1 lists of joint_cap + 1 integers, or None without pairs)"""
    raw, rb, N = as_bytes(body), row_bytes(key_words, n_cols, mode), n_cols
    assert len(raw) % rb == 0
    cols = list(range(N)) if cols is None else [int(c) for c in cols]
    hist = [[0] * (cap + 2) for _ in cols]
    pairs = None if pairs is None else [(int(x), int(y)) for x, y in pairs]
    W = joint_cap + 1
    joint = None if pairs is None else [[[0] * W for _ in range(W)] for _ in pairs]
    for r in range(len(raw) // rb):
        pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
        if mode == MODE_COUNT:
            v = struct.unpack(f"<{N}I", pay)
        else:
            bits = int.from_bytes(pay, "little")      # (the padding bits above N are never looked at)
            v = [(bits >> i) & 1 for i in range(N)]
        for j, c in enumerate(cols):
            x = v[c]
            if x >= cap:
                hist[j][cap] += 1
                hist[j][cap + 1] += x
            else:
                hist[j][x] += 1
        if pairs is not None:
            for p, (x, y) in enumerate(pairs):
                a, b = v[x], v[y]
                joint[p][a if a < joint_cap else joint_cap][b if b < joint_cap else joint_cap] += 1
    return hist, joint


# ---- road 2: numpy over whole columns ---------------------------------------------------------------------------------------------
def hist_expected_np(body, n_cols, key_words, mode, cols=None, cap=255):
    """-> uint64 [M, cap + 2]"""
    cols = np.arange(n_cols) if cols is None else np.asarray(cols, np.int64)
    pay = split_payload(body, n_cols, key_words, mode)
    hist = np.zeros((len(cols), cap + 2), np.uint64)
    for j, c in enumerate(cols):
        v = pay[:, c].astype(np.uint64)
        hist[j, :cap + 1] = np.bincount(np.minimum(v, cap).astype(np.int64), minlength=cap + 1)
        hist[j, cap + 1] = v[v >= cap].sum(dtype=np.uint64)
    return hist


def joint_expected_np(body, n_cols, key_words, mode, pairs, joint_cap=63):
    """-> uint64 [P, joint_cap + 1, joint_cap + 1]"""
    pay = split_payload(body, n_cols, key_words, mode)
    W = joint_cap + 1
    folded = {}
    joint = np.zeros((len(pairs), W, W), np.uint64)
    for p, (x, y) in enumerate(pairs):
        for c in (int(x), int(y)):
            if c not in folded:
                folded[c] = np.minimum(pay[:, c].astype(np.int64), joint_cap)
        joint[p] = np.bincount(folded[int(x)] * W + folded[int(y)], minlength=W * W).reshape(W, W)
    return joint


def spectra_expected_np(body, n_cols, key_words, mode, cols=None, cap=255, pairs=None, joint_cap=63):
    return hist_expected_np(body, n_cols, key_words, mode, cols, cap), None if pairs is None else joint_expected_np(body, n_cols, key_words, mode, pairs, joint_cap)


# ---- the launcher's plan of the pairs, for algo_bytes (kmx.h states the formula) ------------------------------------------------------
def joint_plan(pairs, joint_cap, rb):
    """-> dict(G, n_groups, U, sum_u, lds, stream)"""
    cells = (joint_cap + 1) ** 2
    lds = joint_cap <= JOINT_LDS_CAP
    G = min(GROUP, JOINT_LDS_WORDS // cells) if lds else GROUP
    us = [len({int(c) for pr in pairs[g:g + G] for c in pr}) for g in range(0, len(pairs), G)]
    return dict(G=G, n_groups=len(us), U=max(us), sum_u=sum(us), lds=lds, stream=256 * max(us) > rb)


def algo_bytes(n_rows, n_cols, key_words, mode, n_use=0, cap=None, pairs=None, joint_cap=None):
    rb = row_bytes(key_words, n_cols, mode)
    b = 0
    if cap is not None:
        b += n_rows * rb + 8 * n_use * (cap + 2)
    if pairs is not None:
        pl = joint_plan(pairs, joint_cap, rb)
        b += (pl["n_groups"] * n_rows * rb if pl["stream"] else n_rows * (4 if mode == MODE_COUNT else 1) * pl["sum_u"]) + 8 * len(pairs) * (joint_cap + 1) ** 2
    return b


# ---- the statistics of the driver, exact --------------------------------------------------------------------------------------------
def sample_stats(h, cap):
    """h: a line of hist, cap + 2 integers -> dict of integers"""
    h = [int(x) for x in h]
    valley = next((b for b in range(1, cap - 1) if h[b] < h[b + 1]), 0)
    rng = range(valley + 1, cap)
    peak = max(rng, key=lambda b: (h[b], -b)) if len(rng) else 0
    return dict(rows=sum(h[1:cap + 1]), singletons=h[1], volume=sum(b * h[b] for b in range(cap)) + h[cap + 1], tail_volume=h[cap + 1], valley=valley, peak=peak)


def pair_stats(J, joint_cap, solid=1, k=None):
    """J: a pair's table -> dict: both, x_only, y_only integers; jaccard, completeness Fractions or None (0 / 0); qv a float, math.inf,
    math.nan, or None without k"""
    J = [[int(x) for x in row] for row in J]
    W = joint_cap + 1
    both = sum(J[a][b] for a in range(1, W) for b in range(1, W))
    x_only, y_only = sum(J[a][0] for a in range(1, W)), sum(J[0][b] for b in range(1, W))
    union = both + x_only + y_only
    den = sum(J[a][b] for a in range(solid, W) for b in range(W))
    num = sum(J[a][b] for a in range(solid, W) for b in range(1, W))
    qv = None
    if k is not None:
        E, K = y_only, both + y_only
        if K == 0:
            qv = math.nan
        elif E == 0:
            qv = math.inf
        else:      # 1 - (1 - E/K)^(1/k), without cancellation: -expm1(log1p(-E/K) / k); E = K: the error rate is 1
            qv = -10 * math.log10(-math.expm1(math.log1p(-E / K) / k)) if E < K else 0.0
    return dict(both=both, x_only=x_only, y_only=y_only, jaccard=Fraction(both, union) if union else None,
                completeness=Fraction(num, den) if den else None, qv=qv)


# ---- the driver's texts ---------------------------------------------------------------------------------------------------------------
def hist_text(ids, cap, hist):
    lines = ["# kmx spectra hist", f"# samples: {len(ids)}", f"# cap: {cap}"] + [f"# id: {s}" for s in ids] + ["bin" + "".join(f"\t{j}" for j in range(len(ids)))]
    lines += ["\t".join([str(b)] + [str(int(hist[j][b])) for j in range(len(ids))]) for b in range(cap + 1)]
    lines += ["\t".join(["volume"] + [str(int(hist[j][cap + 1])) for j in range(len(ids))])]
    return "\n".join(lines) + "\n"


def joint_text(id_pairs, joint_cap, joint):
    lines = ["# kmx spectra joint", f"# pairs: {len(id_pairs)}", f"# cap: {joint_cap}"] + [f"# pair: {x}\t{y}" for x, y in id_pairs] + ["pair\ta\tb\trows"]
    for p in range(len(id_pairs)):
        for a, b in np.argwhere(np.asarray(joint[p]) != 0):
            lines.append(f"{p}\t{a}\t{b}\t{int(joint[p][a][b])}")
    return "\n".join(lines) + "\n"


SAMPLE_COLUMNS = "sample\trows\tsingletons\tvolume\ttail_volume\tvalley\tpeak"
PAIR_COLUMNS = "x\ty\tboth\tx_only\ty_only\tjaccard\tcompleteness\tqv"


def parse_report(text):
    """the text `kmx spectra` prints -> (head dict, sample lines [(id, rows, singletons, volume, tail_volume, valley, peak)], pair
    lines [(x, y, both, x_only, y_only, jaccard, completeness, qv)] with the last three as the strings printed)"""
    lines = text.splitlines()
    assert lines[0] == "# kmx spectra"
    head, i = {}, 1
    while lines[i].startswith("# "):
        k, v = lines[i][2:].split(": ", 1)
        head[k] = v
        i += 1
    assert list(head) == ["samples", "cap", "pairs", "joint_cap", "solid", "kmer_size"]
    assert lines[i] == SAMPLE_COLUMNS
    M, P = int(head["samples"]), int(head["pairs"])
    samples = []
    for ln in lines[i + 1:i + 1 + M]:
        c = ln.split("\t")
        assert len(c) == 7
        samples.append((c[0],) + tuple(int(x) for x in c[1:]))
    rest = lines[i + 1 + M:]
    pairs = []
    if P:
        assert rest[0] == PAIR_COLUMNS and len(rest) == P + 1
        for ln in rest[1:]:
            c = ln.split("\t")
            assert len(c) == 8
            pairs.append((c[0], c[1], int(c[2]), int(c[3]), int(c[4]), c[5], c[6], c[7]))
    else:
        assert not rest
    return head, samples, pairs


def check_printed(got, exact, digits):
    """a printed ratio against the exact one: within one unit of the last printed digit; 'nan' for 0 / 0"""
    if exact is None or (isinstance(exact, float) and math.isnan(exact)):
        assert got == "nan", got
    elif isinstance(exact, float) and math.isinf(exact):
        assert got == "inf", got
    else:
        a, _, b = got.partition(".")
        assert a.isdigit() and b.isdigit() and len(b) == digits, got
        assert abs(Fraction(got) - Fraction(exact)) <= Fraction(1, 10 ** digits), (got, exact)


def check_report(text, ids, cap, hist, id_pairs, joint_cap, joint, solid, k):
    """the whole report against the exact statistics of the tables"""
    head, samples, pairs = parse_report(text)
    assert head == dict(samples=str(len(ids)), cap=str(cap), pairs=str(len(id_pairs)), joint_cap=str(joint_cap) if id_pairs else "NA",
                        solid=str(solid) if id_pairs else "NA", kmer_size="NA" if k is None else str(k)), head
    for j, line in enumerate(samples):
        s = sample_stats(hist[j], cap)
        assert line == (ids[j], s["rows"], s["singletons"], s["volume"], s["tail_volume"], s["valley"], s["peak"]), (j, line, s)
    for p, line in enumerate(pairs):
        s = pair_stats(joint[p], joint_cap, solid, k)
        assert line[:5] == (id_pairs[p][0], id_pairs[p][1], s["both"], s["x_only"], s["y_only"]), (p, line, s)
        check_printed(line[5], s["jaccard"], 6)
        check_printed(line[6], s["completeness"], 6)
        if k is None:
            assert line[7] == "NA"
        else:
            check_printed(line[7], s["qv"], 4)


# ---- what the GPU test sends ------------------------------------------------------------------------------------------------------
def make_cols(kind, N, seed):
    """the lists of the sweep -> a uint32 array, or None (the identity said by leaving the list out)"""
    if kind == "none":
        return None
    if kind == "reversed":
        return np.arange(N, dtype=np.uint32)[::-1].copy()
    if kind == "one":
        return np.array([N // 2], np.uint32)
    assert kind == "scattered"
    return np.random.default_rng(seed).permutation(N)[:max(1, (2 * N) // 3)].astype(np.uint32)


def make_pairs(kind, N, joint_cap, seed):
    """P pairs of input columns: 'one'; 'g-1', 'g', 'g+1' around the pairs of a group; 'many' 70.  From three pairs on, one has x = y and
    one comes twice"""
    G = joint_plan([(0, 0)], joint_cap, 1 << 40)["G"]
    P = {"one": 1, "g-1": max(1, G - 1), "g": G, "g+1": G + 1, "many": 70}[kind]
    pr = np.random.default_rng(seed).integers(0, N, (P, 2)).astype(np.uint32)
    if P >= 3:
        pr[1, 1] = pr[1, 0]
        pr[P - 1] = pr[0]
    return pr


def spectra_body(seed, n_rows, N, kw, mode, shape, caps=(255, 63)):
    """'zero': all-zero rows; 'same': one random row, repeated; 'skewed': nearly every cell 0, the others small; 'uniform': every cell
    drawn alike from 0, small counts, C - 1, C, C + 1 for every C of caps and 2^32 - 1.  PA: every padding bit set."""
    rng = np.random.default_rng(seed)
    pool = np.array(sorted({0, 1, 2, 3, 5, U32} | {max(0, C + d) for C in caps for d in (-1, 0, 1)}), np.uint32)
    rows = 1 if shape == "same" else n_rows
    if shape == "zero":
        c = np.zeros((rows, N), np.uint32)
    elif shape == "skewed":
        c = pool[rng.integers(1, len(pool), (rows, N))]
        c[rng.random((rows, N)) < 0.97] = 0
    else:
        c = pool[rng.integers(0, len(pool), (rows, N))]
    if shape == "same":
        c = np.repeat(c, n_rows, axis=0)
    keys = rng.integers(0, 256, (n_rows, 8 * kw), dtype=np.uint8)
    if mode == MODE_COUNT:
        pay = c.astype("<u4").view(np.uint8).reshape(n_rows, 4 * N)
    else:
        bits = np.concatenate([c != 0, np.ones((n_rows, (-N) % 8), bool)], axis=1)
        pay = np.packbits(bits, axis=1, bitorder="little").reshape(n_rows, (N + 7) // 8)
    return np.ascontiguousarray(np.concatenate([keys, pay], axis=1)).reshape(-1)


class Case:
    def __init__(self, name, mode, n_cols, key_words, n_rows, shape, kind, cap, pair_kind, joint_cap, seed, pairs=None):
        self.name, self.mode, self.n_cols, self.key_words, self.n_rows, self.shape, self.kind = name, mode, n_cols, key_words, n_rows, shape, kind
        self.cap, self.pair_kind, self.joint_cap, self.seed = cap, pair_kind, joint_cap, seed
        self.cols = make_cols(kind, n_cols, seed)
        self.pairs = make_pairs(pair_kind, n_cols, joint_cap, seed + 1) if pairs is None else np.array(pairs, np.uint32)
        self.n_use = n_cols if self.cols is None else len(self.cols)
        self.row_bytes = row_bytes(key_words, n_cols, mode)
        self.plan = joint_plan(self.pairs, joint_cap, self.row_bytes)

    @functools.cached_property
    def body(self):
        b = spectra_body(self.seed, self.n_rows, self.n_cols, self.key_words, self.mode, self.shape, (self.cap, self.joint_cap))
        assert len(b) == self.n_rows * self.row_bytes
        b.setflags(write=False)
        return b

    @functools.cached_property
    def expected(self):
        """the numpy road's word, worked out once: (hist, joint)"""
        return spectra_expected_np(self.body, self.n_cols, self.key_words, self.mode, self.cols, self.cap, self.pairs, self.joint_cap)

    def algo_bytes(self, hist=True, joint=True):
        return algo_bytes(self.n_rows, self.n_cols, self.key_words, self.mode, self.n_use, self.cap if hist else None, self.pairs if joint else None, self.joint_cap)


COLUMNS = [1, 7, 8, 9, 63, 64, 65, 130, 257, 1025]
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 4200]
SHAPES = ["zero", "same", "skewed", "uniform"]
KINDS = ["none", "reversed", "scattered", "one"]
CAPS1 = [1, 2, 255, HIST_LDS_CAP - 1, HIST_LDS_CAP + 1, 65535]
CAPS2 = [1, 2, 63, JOINT_LDS_CAP - 1, JOINT_LDS_CAP, JOINT_LDS_CAP + 1, 255]
PAIR_KINDS = ["one", "g-1", "g", "g+1", "many"]


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """combinations, not the full product: every N in both modes three times over, and every value of the other axes -- rows, key
    words, body shapes, lists, both caps, pair counts -- rotating at strides that are coprime to each other; the largest tables ride on
    the narrower matrices (cap 65535 on at most 130 listed columns, 70 pairs at a joint cap of 63 at the most).  Then the long bodies in
    every shape on one block and on several, and both roads of JOINT on either side of the rule (test_spectra_cpu asserts the
    coverage)"""
    cases = []
    i = 0
    for rep in range(3):
        for N in COLUMNS:
            for mode in (MODE_COUNT, MODE_PA):
                n, d = i // 2, i % 2      # (the mode alternates with i: every axis turns with n, and starts elsewhere in the other mode)
                rows = ROWS[(n * 2 + rep + d * 4) % len(ROWS)]
                if mode == MODE_COUNT and N == 1025 and rows > 257:
                    rows = 257      # (a few MB at the most)
                kw = 1 + (n + d) % 4
                shape = SHAPES[(n + rep + d) % len(SHAPES)]
                kind = KINDS[(n + n // 4 + d) % len(KINDS)]
                cap = CAPS1[(n + d * 3) % len(CAPS1)]
                if cap == 65535 and N > 130:
                    kind = "one"
                jc = CAPS2[(n * 3 + rep + d * 2) % len(CAPS2)]
                pk = PAIR_KINDS[(n + n // 5 + d) % len(PAIR_KINDS)]
                if pk == "many" and jc > 63:
                    pk = "g+1"
                m = "c" if mode == MODE_COUNT else "p"
                cases.append(Case(f"{m}-{N}-{kind}-r{rows}-k{kw}-{shape}-c{cap}-{pk}-j{jc}", mode, N, kw, rows, shape, kind, cap, pk, jc, 7000 + i))
                i += 1
    # the long bodies in every shape: several runs of rows a block, several blocks
    for mode in (MODE_COUNT, MODE_PA):
        for N, shape, kind, cap, pk, jc in ((9, "same", "none", 255, "g", 63), (65, "uniform", "reversed", 255, "many", 2), (130, "skewed", "scattered", 256, "one", 110),
                                            (64, "zero", "none", 2, "g+1", 109), (257, "uniform", "scattered", 254, "g-1", 63), (130, "uniform", "none", 65535, "one", 255)):
            m = "c" if mode == MODE_COUNT else "p"
            cases.append(Case(f"{m}-{N}-{kind}-r4200-k1-{shape}-c{cap}-{pk}-j{jc}-long", mode, N, 1, 4200, shape, kind, cap, pk, jc, 7500 + len(cases)))
    # either side of the rule that picks JOINT's road: rows of 528 bytes gather two columns (512 <= 528) and stream three; PA rows long
    # enough to gather at all; rows that differ by a byte around 512 = 256 * 2
    for mode, N, kw, pairs, jc, tag in ((MODE_COUNT, 130, 1, [(3, 129)], 2, "u2"), (MODE_COUNT, 130, 1, [(3, 129), (3, 64)], 2, "u3"), (MODE_PA, 4200, 1, [(4199, 0)], 2, "u2"),
                                        (MODE_PA, 4200, 1, [(4199, 0), (7, 8)], 2, "u4"), (MODE_PA, 4025, 1, [(4024, 9)], 2, "rb512"), (MODE_PA, 4017, 1, [(4016, 9)], 2, "rb511"),
                                        (MODE_PA, 2100, 3, [(2099, 2099)], 2, "u1"), (MODE_PA, 4200, 2, [(4199, 0)], 255, "u2"), (MODE_COUNT, 130, 2, [(129, 0)], 110, "u2")):
        m = "c" if mode == MODE_COUNT else "p"
        cases.append(Case(f"{m}-{N}-one-r700-k{kw}-uniform-c2-rule-j{jc}-{tag}", mode, N, kw, 700, "uniform", "one", 2, "rule", jc, 7700 + len(cases), pairs))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
