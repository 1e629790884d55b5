"""`kmx diff` on the MI355X against tests/diff_ref.py: the C ABI through kmtricks_amd.lib on the bodies of diff_ref.gpu_cases() -- the
integers of every record, the kept body and the column sums exactly, the statistic within the derived tolerance of the mpmath road, the
keep set exactly (tests/test_diff_cpu.py shows that no row of these inputs lies in the tolerance band) --, and the driver on the golden
samples.  Run with -m gpu."""
import ctypes as C
import math
import os, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr
import diff_ref as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = fr.MODE_COUNT, fr.MODE_PA
WORST = {"units": 0.0, "where": None}      # the largest |stat - mpmath| seen, in units of 2^-53 * sum c_g (1 + |ln r_g|) (tol = 16 units)


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def compare(out, c, thr, min_rec, what):
    """a DiffOutput against the judge's rows of case c"""
    rb = dr.row_bytes(c.key_words, c.n_cols, c.mode)
    kept, band = fr.keep_expected(c.rows, thr, min_rec)
    assert not any(band), what
    idx = [i for i, k in enumerate(kept) if k]
    got = out.recs
    assert got["row"].tolist() == idx, f"{what}: kept rows {got['row'].tolist()[:8]} ... ({len(got)}), expected {idx[:8]} ... ({len(idx)})"
    for name, key in (("sum_ctrl", "c0"), ("sum_case", "c1"), ("rec_ctrl", "r0"), ("rec_case", "r1"), ("over", "over")):
        assert got[name].tolist() == [c.rows[i][key] for i in idx], f"{what}: {name}"
    for q, i in zip(got, idx):
        x = c.rows[i]
        err = abs(x["stat"] - float(q["stat"]))
        assert err <= x["tol"], f"{what}: row {i}: stat {float(q['stat'])!r}, expected {float(x['stat'])!r} within {float(x['tol'])!r}"
        if x["tol"]:
            units = float(err / x["tol"]) * 16
            if units > WORST["units"]:
                WORST.update(units=units, where=(what, i))
    src = np.asarray(c.body).reshape(-1, rb) if c.n_rows else np.zeros((0, rb), np.uint8)
    assert out.body == src[idx].tobytes(), f"{what}: the kept body"
    assert out.algo_bytes == c.n_rows * rb + len(idx) * (rb + 40), what
    return idx


def run_case(ctx, c, thr, min_rec=None):
    min_rec = c.min_rec if min_rec is None else min_rec
    out = ctx.diff(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, c.group, c.totals[0], c.totals[1], thr, min_rec)
    return out, compare(out, c, thr, min_rec, f"{c.name} thr={thr!r} min_rec={min_rec}")


@pytest.mark.parametrize("name", [c.name for c in fr.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of the byte and of a wave's worth of units; rows on both sides of a wave's chunk and of a placement tile;
    key widths and PA rows at every alignment; zeros, 0xFF bytes, ignored columns; thresholds 0, p = 0.05, +inf and chosen shares"""
    c = fr.case(name)
    for thr in c.thresholds:
        out, idx = run_case(ctx, c, thr)
        if thr == 0.0:
            assert idx == list(range(c.n_rows))
        if math.isinf(thr):
            assert idx == [] and out.body == b""
        assert all(a < b for a, b in zip(out.recs["row"][:-1], out.recs["row"][1:]))      # file order


def test_extremes(ctx):
    for m in ("count", "pa"):
        z = fr.case(f"zeros-{m}")
        out, idx = run_case(ctx, z, 0.0)
        assert len(idx) == z.n_rows and not out.recs["stat"].any() and not out.recs["over"].any()
        assert run_case(ctx, z, 1.0)[1] == []
        ig = fr.case(f"ignored-{m}")
        out, idx = run_case(ctx, ig, 0.0)
        assert len(idx) == ig.n_rows and not out.recs["sum_ctrl"].any() and not out.recs["rec_case"].any()
        assert run_case(ctx, ig, 0.0, min_rec=1)[1] == []
    big = fr.case("ones-count-own")
    out, _ = run_case(ctx, big, 0.0)
    assert int(out.recs["sum_ctrl"][0]) == int((big.group == 0).sum()) * 0xFFFFFFFF and int(out.recs["sum_case"][69]) == int((big.group == 1).sum()) * 0xFFFFFFFF
    s = ctx.colsums(big.body, None, 1000, 1, COUNT)
    assert s.tolist() == [70 * 0xFFFFFFFF] * 1000


def test_kept_shares(ctx):
    for m in ("count", "pa"):
        c = fr.case(f"shares-{m}")
        n = [len(run_case(ctx, c, t)[1]) for t in c.thresholds]
        assert 2 <= n[0] <= 12 and 1800 <= n[1] <= 2400 and n[2] == 4000, n


@pytest.mark.parametrize("name", ["cols-count-9", "cols-pa-100", "cols-count-1000"])
def test_min_rec(ctx, name):
    """min_rec at r0 + r1 - 1, r0 + r1 and r0 + r1 + 1 of a chosen row"""
    c = fr.case(name)
    j = next(i for i, x in enumerate(c.rows) if x["r0"] + x["r1"] >= 2 and any(y["r0"] + y["r1"] != x["r0"] + x["r1"] for y in c.rows))
    r = c.rows[j]["r0"] + c.rows[j]["r1"]
    got = [j in run_case(ctx, c, 0.0, min_rec=mr)[1] for mr in (r - 1, r, r + 1)]
    assert got == [True, True, False]
    run_case(ctx, c, fr.threshold(fr.P05), min_rec=r)      # (a pair of test_case's list: no row in the band)


@pytest.mark.parametrize("name", ["cols-count-9", "cols-count-100", "cols-pa-9", "cols-pa-1000", "rows-count-70-773", "rows-pa-5-773", "keys-pa-3"])
def test_host_and_device_resident_give_the_same_bits(ctx, name):
    """through _host and through _dev, from a body at any device address: the same records, bit for bit, and the same body"""
    import torch
    c = fr.case(name)
    thr = fr.threshold(fr.P05)      # (among the case's thresholds)
    assert thr in c.thresholds
    host, _ = run_case(ctx, c, thr)
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 3):
        buf = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        buf[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        out = ctx.diff_dev(buf.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, c.group, c.totals[0], c.totals[1], thr, c.min_rec)
        assert out.recs.tobytes() == host.recs.tobytes() and out.body == host.body and out.algo_bytes == host.algo_bytes, (name, shift)
        s = ctx.colsums_dev(buf.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode)
        assert np.array_equal(s, fr.colsums_np(c.body, c.n_cols, c.key_words, c.mode))


@pytest.mark.parametrize("name", ["rows-count-5-65", "rows-count-70-65", "rows-pa-5-65", "rows-pa-70-65"])
def test_a_row_alone_and_among_many(ctx, name):
    """the statistic of a row is the same bits in a call of one row and in a call of many, and at every position in a wave"""
    c = fr.case(name)
    rb = dr.row_bytes(c.key_words, c.n_cols, c.mode)
    many, _ = run_case(ctx, c, 0.0)
    body = np.asarray(c.body).reshape(-1, rb)
    for r in range(c.n_rows):
        one = ctx.diff(body[r].copy(), 1, c.n_cols, c.key_words, c.mode, c.group, c.totals[0], c.totals[1], 0.0)
        a, b = one.recs[0].copy(), many.recs[r].copy()
        assert a["row"] == 0 and b["row"] == r
        a["row"] = b["row"]
        assert a.tobytes() == b.tobytes() and one.body == body[r].tobytes(), (name, r)
    # one row's bytes at 130 places: every lane of a wave, and the waves of a tile
    j = max(range(c.n_rows), key=lambda i: float(c.rows[i]["stat"]))
    rep = np.tile(body[j], 130)
    out = ctx.diff(rep, 130, c.n_cols, c.key_words, c.mode, c.group, c.totals[0], c.totals[1], 0.0)
    assert out.recs["row"].tolist() == list(range(130)) and len(set(out.recs["stat"].tobytes()[i * 8:i * 8 + 8] for i in range(130))) == 1
    assert out.recs["stat"][0].tobytes() == many.recs["stat"][j].tobytes() and float(many.recs["stat"][j]) > 0


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_colsums(ctx, mode):
    """every column shape; one call equals the sum of calls over arbitrary cuts; the sums accumulate into a caller's table; no rows add
    nothing"""
    import torch
    m = "count" if mode == COUNT else "pa"
    for N in (2, 7, 8, 9, 63, 64, 65, 100, 128, 129, 1000):
        c = fr.case(f"cols-{m}-{N}")
        s = ctx.colsums(c.body, None, N, 1, mode)
        assert np.array_equal(s, fr.colsums_np(c.body, N, 1, mode)), N
    for name in (f"shares-{m}", f"rows-{m}-70-773", f"keys-{m}-3", f"rows-{m}-5-0"):
        c = fr.case(name)
        N, kw = c.n_cols, c.key_words
        rb = dr.row_bytes(kw, N, mode)
        exp = fr.colsums_np(c.body, N, kw, mode)
        whole = ctx.colsums(c.body, c.n_rows, N, kw, mode)
        assert np.array_equal(whole, exp), name
        table = torch.zeros(N, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        cuts = sorted({0, 1, c.n_rows // 3, c.n_rows // 3, (2 * c.n_rows) // 3 + 1, c.n_rows} & set(range(c.n_rows + 1)))
        for series in (1, 2):
            for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
                out = ctx.colsums(np.asarray(c.body)[a * rb:b * rb], b - a, N, kw, mode, sums_dev=table.data_ptr())
            ctx.colsums(b"", 0, N, kw, mode, sums_dev=table.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(table.cpu().numpy().view(np.uint64), series * exp), (name, series)
        r = ctx.colsums(c.body, c.n_rows, N, kw, mode, keep=True)
        try:
            assert r.sums_dev() and r.algo_bytes() == c.n_rows * rb + 8 * N
        finally:
            r.free()


@pytest.mark.parametrize("N", [2049, 4100])
def test_colsums_of_wide_pa_rows(ctx, N):
    """presence/absence rows of more than 256 payload bytes: k_colsums<PA> takes them in two and three blocks of 256 bytes (grid x);
    every padding bit set; one call, and calls over cuts that accumulate into a caller's table"""
    import torch
    rows, kw = 150, 1 + N % 4
    rb = dr.row_bytes(kw, N, PA)
    assert (N + 7) // 8 > 256
    body = fr.make_body(N, rows, N, kw, PA, fill=0.4, pad_ones=True)
    assert (body.reshape(rows, rb)[:, -1] >> (N % 8)).min() == (0xFF >> (N % 8))
    exp = fr.colsums_np(body, N, kw, PA)
    assert exp[-1] > 0 and exp[2048] > 0 and len(set(exp.tolist())) > 10
    assert np.array_equal(ctx.colsums(body, rows, N, kw, PA), exp)
    table = torch.zeros(N, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    cuts = [0, 1, 50, 101, rows]
    for series in (1, 2):
        for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
            ctx.colsums(body[a * rb:b * rb], b - a, N, kw, PA, sums_dev=table.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(table.cpu().numpy().view(np.uint64), series * exp), series


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    c = fr.case("cols-count-9")
    grp = np.array(c.group)

    def call(code, kw=1, mode=COUNT, N=9, group=grp, T0=5, T1=7, thr=1.0, n_rows=0, sums=True):
        g = np.ascontiguousarray(group, np.uint8)
        for fn in (lib._lib.kmx_diff_host, lib._lib.kmx_diff_dev):
            t = lib.KmxDiffTask(kw, mode, N, 0, None, n_rows, g.ctypes.data, T0, T1, thr)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, T0, T1, thr)
        if sums:
            for fn in (lib._lib.kmx_colsums_host, lib._lib.kmx_colsums_dev):
                t = lib.KmxColsumsTask(kw, mode, N, 0, None, n_rows, None)
                res = C.c_void_p()
                assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N)

    INVAL, UNSUP = -2, -5
    call(INVAL, N=0)
    call(INVAL, mode=7)
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, group=np.where(np.arange(9) == 4, 3, grp), sums=False)
    call(INVAL, group=np.where(grp == 0, 2, grp), sums=False)      # no control column
    call(INVAL, group=np.where(grp == 1, 2, grp), sums=False)      # no case column
    call(INVAL, T0=0, sums=False); call(INVAL, T1=0, sums=False)
    call(INVAL, thr=math.nan, sums=False); call(INVAL, thr=-1e-300, sums=False); call(INVAL, thr=-math.inf, sums=False)
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode)
    big = np.zeros(2 ** 30, np.uint8); big[1] = 1
    call(UNSUP, N=2 ** 30, group=big)                               # a row of 8 + 2^32 bytes
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32, mode=PA)
    # the context stays usable
    run_case(ctx, c, fr.threshold(fr.P05))
    assert np.array_equal(ctx.colsums(c.body, None, 9, 1, COUNT), fr.colsums_np(c.body, 9, 1, COUNT))


def test_worst_statistic_error_is_inside_the_tolerance(ctx):
    """(prints the figure DESIGN section 15 records; runs after the cases above)"""
    for c in fr.gpu_cases():
        if c.name.startswith(("cols-", "ones-")):
            run_case(ctx, c, 0.0)
    print(f"\nlargest statistic error on the device: {WORST['units']:.3f} units of 2^-53 * sum c_g (1 + |ln r_g|) at {WORST['where']} (tolerance: 16)")
    assert WORST["units"] <= 16


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def kmer_string(key, k):
    w = int.from_bytes(bytes(key), "little")
    return "".join("ACTG"[(w >> (2 * (k - 1 - i))) & 3] for i in range(k))


def expected_lines(run, mode, group, thr, k=31, n_parts=4):
    """-> the fields of every line `kmx diff --counts` prints for the run: [key, label, p, stat, integers ...]"""
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, n_parts, k)
    sums = sum(fr.colsums_np(b, n, kw, rmode) for b in bodies)
    T0, T1 = fr.totals_of(sums, group)
    rb = dr.row_bytes(kw, n, rmode)
    lines = []
    for b in bodies:
        rows = fr.diff_expected_py(b, n, kw, rmode, list(group), T0, T1)
        kept, band = fr.keep_expected(rows, thr)
        assert not any(band)
        pay = dr.split_payload(b, n, kw, rmode)
        for i, x in enumerate(rows):
            if kept[i]:
                key = np.asarray(b)[i * rb:i * rb + 8 * kw]
                name = kmer_string(key, k) if mode.startswith("kmer") else str(int.from_bytes(bytes(key), "little"))
                s = float(x["stat"])
                lines.append([name, ("none", "case", "control")[x["over"]], fr.pvalue(s), s] +
                             [str(v) for v in (x["c0"], x["c1"], x["r0"], x["r1"])] + [str(int(v)) for v in pay[i]])
    return lines, (T0, T1)


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples, 4 partitions, with the fixture's repartition table"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxdiff")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    with open(d / "groups.txt", "w") as f:
        f.write("D1 control\nD2\tcase\n")
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    runs = {}
    for mode in ("kmer:count:bin", "kmer:pa:bin"):
        run = d / mode.replace(":", "_")
        r = kmx(*base, "--run-dir", run, "--mode", mode)
        assert r.returncode == 0, r.stderr
        runs[mode] = run
    return dict(dir=d, runs=runs, groups=d / "groups.txt")


@pytest.mark.parametrize("mode", ["kmer:count:bin", "kmer:pa:bin"])
@pytest.mark.parametrize("alpha", [0.05, 0.9])
def test_driver_matches_the_restatement(golden_runs, mode, alpha, tmp_path):
    run = golden_runs["runs"][mode]
    lines, totals = expected_lines(run, mode, (0, 1), fr.threshold(alpha))
    r = kmx("diff", "--run", run, "--groups", golden_runs["groups"], "--correction", "none", "--alpha", alpha, "--counts")
    assert r.returncode == 0, r.stderr
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert got[0] == ["kmer", "over", "pvalue", "stat", "sum_ctrl", "sum_case", "rec_ctrl", "rec_case", "D1", "D2"]
    assert len(got) - 1 == len(lines) and (alpha < 0.5 or len(lines) > 0)
    for g, e in zip(got[1:], lines):
        assert g[:2] == e[:2] and g[4:] == e[4:], (g, e)
        assert g[2] == "%.6e" % float(g[2]) and g[3] == "%.6f" % float(g[3])
        for a, b in ((float(g[2]), e[2]), (float(g[3]), e[3])):
            assert abs(a - b) <= 1e-6 * abs(b), (g, e)
    # --gpus 1 said aloud, and a file as the place: the same bytes; without --counts the same lines without the counts
    r1 = kmx("diff", "--run", run, "--groups", golden_runs["groups"], "--correction", "none", "--alpha", alpha, "--counts", "--gpus", 1, "--output", tmp_path / "o.tsv")
    assert r1.returncode == 0 and r1.stdout == "" and open(tmp_path / "o.tsv").read() == r.stdout, r1.stderr
    r2 = kmx("diff", "--run", run, "--groups", golden_runs["groups"], "--correction", "none", "--alpha", alpha, "--gpus", 2, "-v")
    assert r2.returncode == 0 and r2.stdout.splitlines() == ["\t".join(ln.split("\t")[:8]) for ln in r.stdout.splitlines()], r2.stderr
    assert f"totals {totals[0]} (control) {totals[1]} (case)" in r2.stderr


def test_driver_bonferroni_and_min_rec(golden_runs):
    """Bonferroni divides alpha by the number of rows; --min-rec 2 keeps the rows both samples hold"""
    run = golden_runs["runs"]["kmer:count:bin"]
    bodies, n, kw, rmode = dr.read_run_bodies(run, "kmer:count:bin", 4, 31)
    M = sum(len(b) // dr.row_bytes(kw, n, rmode) for b in bodies)
    lines, _ = expected_lines(run, "kmer:count:bin", (0, 1), fr.threshold(0.9 / M))
    r = kmx("diff", "--run", run, "--groups", golden_runs["groups"], "--alpha", 0.9)
    assert r.returncode == 0 and [ln.split("\t")[0] for ln in r.stdout.splitlines()[1:]] == [e[0] for e in lines], r.stderr
    all_lines, _ = expected_lines(run, "kmer:count:bin", (0, 1), 0.0)
    assert len(all_lines) == M
    r = kmx("diff", "--run", run, "--groups", golden_runs["groups"], "--correction", "none", "--alpha", 0.999999, "--min-rec", 2)
    thr = fr.threshold(0.999999)
    want = [e[0] for e in all_lines if e[6] != "0" and e[7] != "0" and e[3] >= thr]
    assert r.returncode == 0 and [ln.split("\t")[0] for ln in r.stdout.splitlines()[1:]] == want, r.stderr
