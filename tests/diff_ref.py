"""The definition of `kmx diff` (include/kmx.h, section "diff") restated for the tests, by two roads that share no code: plain Python
integers row by row with the statistic in mpmath at 50 digits (diff_expected_py), and numpy with the statistic in float64
(diff_expected_np).  Beside them the column sums by both roads, the driver's threshold (the same bisection on math.erfc), the derived
tolerance of the statistic, and the list of bodies and thresholds that tests/test_diff_gpu.py sends to the device: tests/test_diff_cpu.py
walks the same list and asserts that no row of it lies inside the tolerance band of its threshold."""
import functools
import math
import struct
import numpy as np

from dist_ref import MODE_COUNT, MODE_PA, row_bytes, as_bytes, split_payload

CTRL, CASE, IGN = 0, 1, 2
DIFF_REC = np.dtype([("sum_ctrl", "<u8"), ("sum_case", "<u8"), ("stat", "<f8"), ("rec_ctrl", "<u4"), ("rec_case", "<u4"),
                     ("row", "<u4"), ("over", "<u4")])


# ---- road 1: Python integers and mpmath, row by row -------------------------------------------------------------------------------
def row_counts_py(raw, r, n_cols, key_words, mode):
    rb = row_bytes(key_words, n_cols, mode)
    pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
    if mode == MODE_COUNT:
        return struct.unpack(f"<{n_cols}I", pay)
    bits = int.from_bytes(pay, "little")      # column i = bit i & 7 of byte i >> 3 = bit i of the little-endian integer
    return [(bits >> i) & 1 for i in range(n_cols)]      # (the padding bits above N are never looked at)


def colsums_py(body, n_cols, key_words, mode):
    raw, rb = as_bytes(body), row_bytes(key_words, n_cols, mode)
    assert len(raw) % rb == 0
    sums = [0] * n_cols
    for r in range(len(raw) // rb):
        for i, c in enumerate(row_counts_py(raw, r, n_cols, key_words, mode)):
            sums[i] += c
    return sums


def stat_mp(c0, c1, T0, T1):
    """-> (stat, tol) as mpmath numbers at 50 digits; tol = 16 * 2^-53 * sum over g of c_g * (1 + |ln r_g|), r_g = (c_g T) / (c T_g)"""
    import mpmath
    with mpmath.workdps(50):
        c, T = c0 + c1, T0 + T1
        s, w = mpmath.mpf(0), mpmath.mpf(0)
        for cg, Tg in ((c1, T1), (c0, T0)):
            if cg:
                ln = mpmath.log(mpmath.mpf(cg * T) / mpmath.mpf(c * Tg))
                s += cg * ln
                w += cg * (1 + abs(ln))
        s = 2 * s
        return (s if s > 0 else mpmath.mpf(0)), 16 * mpmath.mpf(2) ** -53 * w


def over_of(c0, c1, T0, T1):
    a, b = c1 * T0, c0 * T1
    return 1 if a > b else 2 if a < b else 0


def diff_expected_py(body, n_cols, key_words, mode, group, T0, T1):
    """-> one dict a row: c0, c1, r0, r1, over (Python integers), stat and tol (mpmath)"""
    raw, rb = as_bytes(body), row_bytes(key_words, n_cols, mode)
    assert len(raw) % rb == 0 and len(group) == n_cols
    out = []
    for r in range(len(raw) // rb):
        counts = row_counts_py(raw, r, n_cols, key_words, mode)
        c, rec = [0, 0, 0], [0, 0, 0]
        for i, v in enumerate(counts):
            c[group[i]] += v
            rec[group[i]] += 1 if v else 0
        s, tol = stat_mp(c[0], c[1], T0, T1)
        out.append(dict(c0=c[0], c1=c[1], r0=rec[0], r1=rec[1], over=over_of(c[0], c[1], T0, T1), stat=s, tol=tol))
    return out


# ---- road 2: numpy ------------------------------------------------------------------------------------------------------------------
def colsums_np(body, n_cols, key_words, mode):
    return split_payload(body, n_cols, key_words, mode).astype(np.uint64).sum(axis=0, dtype=np.uint64)


def stat_np(c0, c1, T0, T1):
    """float64, in the order the header writes the formula"""
    c0, c1 = np.asarray(c0, np.uint64), np.asarray(c1, np.uint64)
    c = (c0 + c1).astype(np.float64)
    T = float(T0 + T1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f1, f0 = c1.astype(np.float64), c0.astype(np.float64)
        t1 = np.where(c1 != 0, f1 * np.log((f1 * T) / (c * float(T1))), 0.0)
        t0 = np.where(c0 != 0, f0 * np.log((f0 * T) / (c * float(T0))), 0.0)
    s = 2.0 * (t1 + t0)
    return np.where(s > 0.0, s, 0.0)


def diff_expected_np(body, n_cols, key_words, mode, group, T0, T1):
    """-> a structured array of DIFF_REC, one entry a row (row = its index)"""
    pay = split_payload(body, n_cols, key_words, mode)
    g = np.asarray(group, np.uint8)
    out = np.zeros(len(pay), DIFF_REC)
    for name, rec, v in (("sum_ctrl", "rec_ctrl", CTRL), ("sum_case", "rec_case", CASE)):
        sel = pay[:, g == v]
        out[name] = sel.astype(np.uint64).sum(axis=1, dtype=np.uint64)
        out[rec] = (sel != 0).sum(axis=1)
    out["row"] = np.arange(len(pay))
    a = out["sum_case"].astype(object) * int(T0)      # exact: Python integers inside
    b = out["sum_ctrl"].astype(object) * int(T1)
    out["over"] = np.where(a > b, 1, np.where(a < b, 2, 0)).astype(np.uint32)
    out["stat"] = stat_np(out["sum_ctrl"], out["sum_case"], T0, T1)
    return out


def diff_expected_mixed(body, n_cols, key_words, mode, group, T0, T1):
    """for the scripts' larger bodies: the integers by the numpy road, the statistic and its tolerance by mpmath -> rows as
    diff_expected_py gives them"""
    q = diff_expected_np(body, n_cols, key_words, mode, group, T0, T1)
    out = []
    for x in q:
        c0, c1 = int(x["sum_ctrl"]), int(x["sum_case"])
        s, tol = stat_mp(c0, c1, T0, T1)
        out.append(dict(c0=c0, c1=c1, r0=int(x["rec_ctrl"]), r1=int(x["rec_case"]), over=over_of(c0, c1, T0, T1), stat=s, tol=tol))
    return out


# ---- the threshold --------------------------------------------------------------------------------------------------------------------
def pvalue(stat):
    return math.erfc(math.sqrt(stat / 2.0))


def threshold(p):
    """the smallest double t in [0, 2000] with erfc(sqrt(t / 2)) <= p: bisection, 200 halvings (what the driver does with std::erfc)"""
    lo, hi = 0.0, 2000.0
    if not pvalue(hi) <= p:
        raise ValueError(f"p = {p} is below what a statistic of 2000 reaches")
    if pvalue(lo) <= p:
        return lo
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if pvalue(mid) <= p:
            hi = mid
        else:
            lo = mid
    return hi


def keep_expected(rows, thr, min_rec=0):
    """rows: diff_expected_py's -> (kept, in_band), a list of booleans each.  A row inside the band |stat - thr| <= tol may go either
    way.  Threshold 0 has no band (stat = max(0, .) is never below it) and +inf none either (a statistic is finite)."""
    kept, band = [], []
    for x in rows:
        ok = x["r0"] + x["r1"] >= min_rec
        if thr == 0.0:
            kept.append(ok); band.append(False)
        elif math.isinf(thr):
            kept.append(False); band.append(False)
        else:
            kept.append(ok and x["stat"] >= thr)
            band.append(ok and abs(x["stat"] - thr) <= x["tol"])
    return kept, band


# ---- bodies ---------------------------------------------------------------------------------------------------------------------------
def make_body(seed, n_rows, n_cols, key_words, mode, fill=0.5, pad_ones=True, maxed=0.0, lo=1, hi=50, group=None, effect=0.0):
    """n_rows rows of random keys and a payload in which a column is present with probability `fill`; PA: every padding bit set
    (pad_ones); COUNT: counts in [lo, hi), a share `maxed` of the present ones 2^32 - 1.  effect (with group): in that share of the
    rows the control columns are absent, so that a few rows stand out.  -> uint8 array"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (n_rows, 8 * key_words), dtype=np.uint8)
    held = rng.random((n_rows, n_cols)) < fill
    if effect and group is not None:
        hit = rng.random(n_rows) < effect
        held[np.ix_(hit, np.asarray(group) == CTRL)] = False
        held[np.ix_(hit, np.asarray(group) == CASE)] = True
    if mode == MODE_COUNT:
        c = rng.integers(lo, hi, (n_rows, n_cols)).astype(np.uint32)
        if maxed:
            c[rng.random((n_rows, n_cols)) < maxed] = 0xFFFFFFFF
        c[~held] = 0
        pay = c.astype("<u4").view(np.uint8).reshape(n_rows, 4 * n_cols)
    else:
        pad = (-n_cols) % 8
        bits = np.concatenate([held, np.full((n_rows, pad), bool(pad_ones))], axis=1)
        pay = np.packbits(bits, axis=1, bitorder="little")
    return np.ascontiguousarray(np.concatenate([keys, pay], axis=1)).reshape(-1)


def clear_columns(body, n_cols, key_words, mode, cols):
    """the body with these columns absent in every row"""
    a = np.array(body, np.uint8).reshape(-1, row_bytes(key_words, n_cols, mode))
    for c in cols:
        if mode == MODE_COUNT:
            a[:, 8 * key_words + 4 * c:8 * key_words + 4 * c + 4] = 0
        else:
            a[:, 8 * key_words + (c >> 3)] &= 0xFF ^ (1 << (c & 7))
    return a.reshape(-1)


def random_groups(seed, n_cols):
    """all three values present when there are three columns; a control and a case always"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, n_cols).astype(np.uint8)
    g[rng.permutation(n_cols)[:min(3, n_cols)]] = [CTRL, CASE, IGN][:min(3, n_cols)]
    return g


def totals_of(sums, group):
    g = np.asarray(group)
    s = [int(x) for x in sums]
    return sum(s[i] for i in range(len(s)) if g[i] == CTRL), sum(s[i] for i in range(len(s)) if g[i] == CASE)


# ---- what the GPU test sends: one list, walked by both test files --------------------------------------------------------------------
P05 = 0.05
WIDE_COUNT_COLS = ((1025, 2025), (1100, 2100))      # (N, seed)
RW_ROWS = (131, 300, 700, 1500, 2048 + 77)
RW_SEEDS = {(m, rows): 3000 + 10 * i + j for j, m in enumerate(("count", "pa")) for i, rows in enumerate(RW_ROWS)}


class Case:
    """a body, its groups and totals, and the thresholds it is tested at.  totals None: the body's own column sums by group."""

    def __init__(self, name, mode, n_cols, key_words, n_rows, group, make, totals=None, thresholds=("p05",), min_rec=0):
        self.name, self.mode, self.n_cols, self.key_words, self.n_rows = name, mode, n_cols, key_words, n_rows
        self.group, self._make, self._totals, self._thr, self.min_rec = np.asarray(group, np.uint8), make, totals, thresholds, min_rec

    @functools.cached_property
    def body(self):
        b = self._make()
        assert len(b) == self.n_rows * row_bytes(self.key_words, self.n_cols, self.mode)
        b.setflags(write=False)
        return b

    @functools.cached_property
    def totals(self):
        if self._totals is not None:
            return self._totals
        return totals_of(colsums_np(self.body, self.n_cols, self.key_words, self.mode), self.group)

    @functools.cached_property
    def rows(self):
        """the judge's word on every row, worked out once"""
        return diff_expected_py(self.body, self.n_cols, self.key_words, self.mode, [int(x) for x in self.group], *self.totals)

    @functools.cached_property
    def thresholds(self):
        """"p05": threshold(0.05); ("top", f): the middle between the statistics of two neighbouring rows in descending order, so that
        a share f of the rows is kept; numbers as they are"""
        out = []
        for t in self._thr:
            if t == "p05":
                out.append(threshold(P05))
            elif isinstance(t, tuple):
                stats = sorted((float(x["stat"]) for x in self.rows), reverse=True)
                k = max(1, round(t[1] * len(stats)))
                while k < len(stats) and stats[k] == stats[k - 1]:      # (between two different statistics)
                    k += 1
                out.append(0.5 * (stats[k - 1] + stats[k]) if k < len(stats) else 0.0)
            else:
                out.append(float(t))
        return out


@functools.lru_cache(maxsize=None)
def gpu_cases():
    cases = []

    def add(name, mode, N, kw, rows, group, totals=None, thresholds=("p05",), min_rec=0, make=None, seed=None, **mk):
        sd = len(cases) + 1000 if seed is None else seed
        g = np.asarray(group, np.uint8)
        cases.append(Case(name, mode, N, kw, rows, g, make or (lambda: make_body(sd, rows, N, kw, mode, group=g, **mk)), totals, thresholds, min_rec))

    for mode in (MODE_COUNT, MODE_PA):
        m = "count" if mode == MODE_COUNT else "pa"
        # columns: both sides of the byte, of a wave's worth of units (64 counts; 64 bytes = 512 bits) and of the 16 units a lane holds
        # (that last edge, 1024 count columns, is WIDE_COUNT_COLS at the end of the list)
        for N in (2, 7, 8, 9, 63, 64, 65, 100, 128, 129, 1000):
            rows = 131 if N == 1000 else 150
            add(f"cols-{m}-{N}", mode, N, 1, rows, random_groups(N, N) if N > 2 else [CTRL, CASE], thresholds=(0.0, "p05", math.inf),
                fill=0.4, maxed=0.02, effect=0.1)
        for N in (9, 65, 130):
            add(f"interleaved-{m}-{N}", mode, N, 1, 150, [i & 1 for i in range(N)], fill=0.4, effect=0.1)
            add(f"all-case-but-one-{m}-{N}", mode, N, 1, 150, [CASE] * (N - 1) + [CTRL], fill=0.4)
        # rows: both sides of a wave's worth of short rows (64) and of a placement tile (256); long rows too (N = 70: a wave a row)
        for rows in (0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 + 5):
            for N in (5, 70):
                add(f"rows-{m}-{N}-{rows}", mode, N, 1, rows, random_groups(rows + N, N), totals=(1000 + rows, 900) if rows < 2 else None,
                    thresholds=(0.0, "p05"), fill=0.5, effect=0.05)
        # key widths; PA rows of 8 kw + 3 bytes (an odd size) start at every alignment
        for kw in (1, 2, 3, 4):
            N = 13 if mode == MODE_COUNT else 21
            add(f"keys-{m}-{kw}", mode, N, kw, 200, random_groups(kw, N), fill=0.5, effect=0.1)
        # every present column in group 2: the rows are as good as empty
        g = [IGN] * 20 + [CTRL, CASE]
        add(f"ignored-{m}", mode, 22, 1, 100, g, totals=(50, 60), thresholds=(0.0, 1.0),
            make=lambda mode=mode: clear_columns(make_body(5, 100, 22, 1, mode, fill=0.7), 22, 1, mode, (20, 21)))
        # a body of zeros: every statistic is 0; a body of 0xFF bytes: counts of 2^32 - 1 in 1000 columns (and every key byte and
        # padding bit set), once with its own totals (every row is the average row) and once with totals that make every row stand out
        add(f"zeros-{m}", mode, 67, 1, 130, random_groups(67, 67), totals=(100, 100), thresholds=(0.0, 1.0, math.inf),
            make=lambda mode=mode: np.zeros(130 * row_bytes(1, 67, mode), np.uint8))
        for tot in (None, (2 ** 45, 2 ** 44 + 12345)):
            add(f"ones-{m}-{'own' if tot is None else 'skewed'}", mode, 1000, 1, 70, random_groups(1000, 1000), totals=tot, thresholds=(0.0, "p05"),
                make=lambda mode=mode: np.full(70 * row_bytes(1, 1000, mode), 0xFF, np.uint8))
        # kept shares: near 0.1 %, 50 % and all, over several tiles
        add(f"shares-{m}", mode, 24, 1, 4000, random_groups(77, 24), thresholds=(("top", 0.001), ("top", 0.5), 0.0), fill=0.3, effect=0.002)
    # (appended behind the cases above, whose seeds follow their place in the list; the seeds below are chosen so that no row lies in
    # the band of its threshold)
    # count columns on both sides of the 16 units a lane of k_diff_score keeps the groups of in a register (64 lanes x 16 = 1024
    # columns): beyond them the group comes from memory, and ignored columns lie there
    for N, sd in WIDE_COUNT_COLS:
        g = random_groups(N, N)
        g[1024] = IGN      # (N = 1025: the one column out there)
        assert N == 1025 or (g[1025:] == CTRL).any() and (g[1025:] == CASE).any() and (g[1025:] == IGN).any()
        add(f"cols-count-{N}", MODE_COUNT, N, 1, 70, g, thresholds=(0.0, "p05", math.inf), seed=sd, fill=0.4, maxed=0.02, effect=0.1)
    # long rows (a wave a row) in every number that gives k_diff_score another chunk of rows when the host plans for one CU
    # (tests/test_launch_shapes_gpu.py): 4, 8, 16, 32 and 64 rows a wave, the last chunk partial, nine placement tiles at the most
    for mode, N in ((MODE_COUNT, 70), (MODE_PA, 520)):
        m = "count" if mode == MODE_COUNT else "pa"
        for i, rows in enumerate(RW_ROWS):
            add(f"rw-{m}-{rows}", mode, N, 1 + (i + mode) % 4, rows, random_groups(rows + N, N), thresholds=(0.0, "p05"),
                seed=RW_SEEDS[(m, rows)], fill=0.5, effect=0.05)
    return cases


def case(name):
    return next(c for c in gpu_cases() if c.name == name)
