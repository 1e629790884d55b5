"""`kmx pca` on the MI355X against tests/gram_ref.py: the C ABI through kmtricks_amd.lib on the bodies of gram_ref.gpu_cases() -- the table
compared bit for bit --, accumulation into the caller's table, the identities against the live Context.pan and Context.dist, the limits,
the launch shapes the two knobs of gram.hip force, and the driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, struct, subprocess
from fractions import Fraction

import numpy as np
import pytest

import dist_ref as dr
import gram_ref as gr
import pan_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = gr.MODE_COUNT, gr.MODE_PA
U32 = gr.U32


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, what):
    assert out.table.dtype == np.uint64 and out.table.shape == exp.shape, what
    assert out.table.tobytes() == exp.tobytes(), f"{what}: first differences at {np.argwhere(out.table != exp)[:3].tolist()}: {out.table[out.table != exp][:3]} for {exp[out.table != exp][:3]}"


def algo_bytes(n_rows, N, kw, mode, words):
    return 2 * n_rows * dr.row_bytes(kw, N, mode) + 16 * n_rows + 2 * 8 * 64 * ((N + 63) // 64) * words + 8 * N * N


@pytest.mark.parametrize("name", [c.name for c in gr.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of a byte, of a block of 64 samples and of a PA lane's span; rows on both sides of a word of the order; every
    row in one class, every class present, classes of exactly 63 / 64 / 65 rows; weights all 1, all 2^32 - 1 (cells pass 2^32), zero for
    some classes and for the largest; lists of every kind; key widths 1 ... 4; PA padding bits all set; counts of 2^32 - 1 with min_abund
    1, 2, 2^32 - 1"""
    c = gr.case(name)
    out = ctx.gram(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, c.weights, cols=c.cols, min_abund=c.abund)
    same(out, c.expected, name)
    assert out.algo_bytes == algo_bytes(c.n_rows, c.n_cols, c.key_words, c.mode, c.words)


ODD = [n for n in (c.name for c in gr.gpu_cases()) if "-edge-" in n][::3] +[n for n in (c.name for c in gr.gpu_cases()) if n.endswith("-long")]


@pytest.mark.parametrize("name", ODD)
def test_body_at_an_odd_host_address_and_device_resident(ctx, name):
    """the body handed in at an odd host address, and through _dev from every device alignment: the same table"""
    import torch
    c = gr.case(name)
    buf = np.zeros(len(c.body) + 9, np.uint8)
    for shift in (1, 3):
        view = buf[shift:shift + len(c.body)]
        view[:] = c.body
        assert view.ctypes.data % 2 == 1
        same(ctx.gram(view, c.n_rows, c.n_cols, c.key_words, c.mode, c.weights, cols=c.cols, min_abund=c.abund), c.expected, (name, "host", shift))
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 3):
        d = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        d[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        same(ctx.gram_dev(d.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, c.weights, cols=c.cols, min_abund=c.abund), c.expected, (name, "dev", shift))


@pytest.mark.parametrize("mode,N,kind", [(COUNT, 65, "scattered"), (PA, 130, "reversed"), (COUNT, 200, "none"), (PA, 9, "one")])
def test_two_calls_into_the_callers_table(ctx, mode, N, kind):
    """one call, against two calls over a cut into a table of the caller's that holds 2^32 - 1 in every cell: an add carries into the
    high word, cells of unlisted columns stay as they were"""
    import torch
    rows, kw, cut = 1500, 2, 389
    body = pr.shaped_body(177 + N, rows, N, kw, mode, "uniform")
    cols = pr.make_cols(kind, N, 5)
    M = N if cols is None else len(cols)
    w = gr.make_weights("holes" if kind != "one" else "ones", M, 3)
    rb = dr.row_bytes(kw, N, mode)
    exp = gr.gram_expected_np(body, N, kw, mode, w, cols)
    same(ctx.gram(body, rows, N, kw, mode, w, cols=cols), exp, "one call")
    dev = torch.device("cuda:0")
    seed = 0xFFFFFFFF
    d_t = torch.full((N, N), seed, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    first = ctx.gram(body[:cut * rb], cut, N, kw, mode, w, cols=cols, table_dev=d_t.data_ptr(), keep=True)
    try:
        assert first.table_dev() == d_t.data_ptr()
        second = ctx.gram(body[cut * rb:], rows - cut, N, kw, mode, w, cols=cols, table_dev=d_t.data_ptr())
    finally:
        first.free()
    torch.cuda.synchronize()
    got = d_t.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, exp + np.uint64(seed))
    assert np.array_equal(second.table, got)      # the table as it stands
    assert (got >> np.uint64(32)).any()           # adds carried
    listed = np.zeros(N, bool)
    listed[np.arange(N) if cols is None else cols] = True
    assert (got[~listed] == seed).all() and (got[:, ~listed] == seed).all()


@pytest.mark.parametrize("mode,N,kind,a", [(COUNT, 70, "scattered", 2), (PA, 130, "none", 1), (COUNT, 64, "reversed", 1), (PA, 65, "scattered", 1)])
def test_identities_against_pan_and_dist(ctx, mode, N, kind, a):
    """(a) the diagonal is the weighted sum of pan's shared table; (c) so is a row's sum, with R more; (b) with the weights (0,1,...,1)
    and min_abund 1 the table is dist's inter on the listed columns -- all three from the device's own pan and dist"""
    rows, kw = 2100, 1
    body = pr.shaped_body(900 + N, rows, N, kw, mode, "uniform")
    cols = pr.make_cols(kind, N, 11)
    M = N if cols is None else len(cols)
    w = gr.make_weights("eigenstrat", M)
    T = ctx.gram(body, rows, N, kw, mode, w, cols=cols, min_abund=a).table
    sh = ctx.pan(body, rows, N, kw, mode, cols=cols, min_abund=a, shared=True).shared
    wi = [int(x) for x in w]
    for i in range(N):
        assert int(T[i][i]) == sum(wi[R] * int(sh[R][i]) for R in range(M + 1))
        assert sum(int(x) for x in T[i]) == sum(R * wi[R] * int(sh[R][i]) for R in range(M + 1))
    if a == 1:
        inter = ctx.dist(body, rows, N, kw, mode).inter
        listed = np.zeros(N, bool)
        listed[np.arange(N) if cols is None else cols] = True
        only = np.zeros_like(inter)
        only[np.ix_(listed, listed)] = inter[np.ix_(listed, listed)]
        assert np.array_equal(ctx.gram(body, rows, N, kw, mode, gr.make_weights("dist", M), cols=cols).table, only)


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    wts = np.ones(2 ** 15 + 2, np.uint32)

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, a=1, flags=0, n_rows=0, weights=True):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        M = (N if cc is None else len(cc)) if M is None else M
        for fn in (lib._lib.kmx_gram_host, lib._lib.kmx_gram_dev):
            t = lib.KmxGramTask(kw, mode, N, M, None, n_rows, None if cc is None else cc.ctypes.data, wts.ctypes.data if weights else None, a, flags, None)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, a, flags, n_rows, weights)

    OK, INVAL, UNSUP = 0, -2, -5
    call(INVAL, N=0, cols=None); call(INVAL, M=0)
    call(INVAL, N=2, cols=(0, 1, 0))                               # n_use > n_cols
    call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4))       # an index at N; a duplicate
    call(INVAL, cols=None, M=8)                                    # the identity with M != N
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, mode=7)
    call(INVAL, a=0); call(INVAL, a=0, mode=PA); call(INVAL, a=2, mode=PA)
    call(INVAL, flags=1); call(INVAL, flags=0x80000000)
    call(INVAL, weights=False)                                     # null weights
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode); call(UNSUP, mode=mode, kw=0)
    call(UNSUP, N=2 ** 30, cols=None)                              # a row of 8 + 2^32 bytes (refused before the weights are looked at)
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32 - 255, mode=PA)
    call(UNSUP, N=2 ** 15 + 1, cols=None); call(UNSUP, N=2 ** 15 + 1, cols=None, mode=PA)      # dist's table limit
    # what is valid is taken: no rows add nothing
    t = lib.KmxGramTask(1, COUNT, 9, 3, None, 0, np.array([4, 2, 1], np.uint32).ctypes.data, wts.ctypes.data, 1, 0, None)
    res = C.c_void_p()
    assert lib._lib.kmx_gram_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
    tb = np.ones((9, 9), np.uint64)
    assert lib._lib.kmx_gram_result_copy_table(res, tb.ctypes.data, tb.size) == OK and not tb.any()
    assert lib._lib.kmx_gram_result_copy_table(res, tb.ctypes.data, tb.size - 1) == INVAL
    assert lib._lib.kmx_gram_result_algo_bytes(res) == 8 * 81
    lib._lib.kmx_gram_result_free(res)
    # the context stays usable
    c = gr.case(next(x.name for x in gr.gpu_cases() if x.name.startswith("c-7-") and x.n_rows))
    same(ctx.gram(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, c.weights, cols=c.cols, min_abund=c.abund), c.expected, c.name)


# ---- the launch shapes KMX_GRAM_CUS and KMX_GRAM_GRID force ----------------------------------------------------------------------
def launch_shape(n_rows, N, M, mode, cus, grid_cap):
    """the launcher's formulas (gram.hip, gram_queue) -> trips of each kernel's stride loop"""
    units = N if mode == COUNT else (N + 7) // 8
    NB = (N + 63) // 64
    L = 1
    while L < 64 and L < units:
        L <<= 1
    RW = 64
    if L == 64:
        while RW > 4 and n_rows // RW < cus * 4 * 8:
            RW >>= 1
    chunks = (n_rows + RW - 1) // RW
    cap = min(1 << 16, grid_cap)
    score_grid = min((chunks + 3) // 4, min(cus * 8, cap))
    tiles = (n_rows + 255) // 256
    order_grid = min(tiles, cap)
    W = n_rows // 64 + min(M + 1, n_rows)
    slab_tiles = W * (NB if mode == COUNT else (NB + 7) // 8)
    slab_grid = min((slab_tiles + 3) // 4, cap)
    pairs = NB * (NB + 1) // 2
    r = max(1, cus * 8 // pairs)
    r = min(r, (W + 63) // 64)
    r = max(r, (W + 2 ** 24 - 1) // 2 ** 24, 1)
    ln = (-(-W // r) + 31) // 32 * 32
    runs = -(-W // ln)
    items = pairs * runs
    pairs_grid = min(items, cap)
    return dict(score=-(-chunks // (4 * score_grid)), order=-(-tiles // order_grid), slab=-(-slab_tiles // (4 * slab_grid)), pairs=-(-items // pairs_grid), runs=runs)


@pytest.mark.parametrize("mode,N,rows,kind", [(COUNT, 300, 2100, "scattered"), (PA, 1100, 2100, "none"), (COUNT, 40, 12001, "reversed"), (PA, 130, 12001, "scattered")])
def test_launch_shapes(ctx, mode, N, rows, kind, monkeypatch):
    """KMX_GRAM_CUS=1 and KMX_GRAM_GRID=3 (read per call): several trips of each stride loop; each shape against the reference and, byte
    for byte, against the same call with the knobs unset"""
    import torch
    kw = 1
    body = pr.shaped_body(2234 + N, rows, N, kw, mode, "uniform")
    cols = pr.make_cols(kind, N, 9)
    M = N if cols is None else len(cols)
    w = gr.make_weights("eigenstrat", M)
    exp = gr.gram_expected_np(body, N, kw, mode, w, cols)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.delenv("KMX_GRAM_CUS", raising=False); monkeypatch.delenv("KMX_GRAM_GRID", raising=False)
    base = ctx.gram(body, rows, N, kw, mode, w, cols=cols)
    same(base, exp, "knobs unset")
    unset = launch_shape(rows, N, M, mode, n_cu, 1 << 16)
    for env in (dict(KMX_GRAM_CUS="1"), dict(KMX_GRAM_GRID="3"), dict(KMX_GRAM_CUS="1", KMX_GRAM_GRID="3")):
        shape = launch_shape(rows, N, M, mode, 1 if "KMX_GRAM_CUS" in env else n_cu, 3 if "KMX_GRAM_GRID" in env else 1 << 16)
        assert shape["score"] > 1, (env, shape)
        if "KMX_GRAM_CUS" in env:
            assert shape["runs"] <= unset["runs"], (env, shape, unset)
        if "KMX_GRAM_GRID" in env:
            assert shape["order"] > 1 and shape["slab"] > 1 and shape["pairs"] > 1, (env, shape)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.gram(body, rows, N, kw, mode, w, cols=cols)
        for k in env:
            monkeypatch.delenv(k)
        same(out, exp, env)
        assert out.table.tobytes() == base.table.tobytes()


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


KINDS = ("kmer:count:bin", "kmer:pa:bin")
IDS = ["D1", "D2", "D3"]


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples and a third made of slices of both, 4 partitions, with the fixture's
    repartition table: every k-mer of every sample is a row"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxpca")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    one, two = (open(os.path.join(GD, f"{i}.fasta")).read().split("\n") for i in (1, 2))
    with open(d / "3.fasta", "w") as f:      # the front of sample 1's first read (twice: counts of 2), the back of sample 2's second, and a read of its own
        f.write(f">a\n{one[1][:70]}\n>b\n{two[3][25:]}\n>c\n{one[3][40:75]}{two[1][10:50]}\n>d\n{one[1][:70]}\n")
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\nD3 : {d}/3.fasta\n")
    base = ["pipeline", "--kmer-size", 31, "--hard-min", 1, "--soft-min", 1, "--recurrence-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    runs = {}
    for mode in KINDS:
        run = d / mode.replace(":", "_")
        r = kmx(*base, "--file", d / "in.fof", "--run-dir", run, "--mode", mode)
        assert r.returncode == 0, r.stderr
        runs[mode] = run
    return dict(dir=d, base=base, runs=runs)


def restated(bodies, n, kw, rmode, cols, a=1, scale="eigenstrat", min_rec=1, max_rec=None):
    """the restatement on a run's bodies, summed over the partitions -> (G exact, magnitudes, F, n_used, rows)"""
    M = n if cols is None else len(cols)
    parts = [pr.pan_expected_np(b, n, kw, rmode, cols, a) for b in bodies]
    spec, sh = sum(p[0] for p in parts), sum(p[1] for p in parts)
    wt, F, used = gr.driver_weights(M, spec[0], scale, min_rec, max_rec)
    T = sum(gr.gram_expected_np(b, n, kw, rmode, wt, cols, a).astype(object) for b in bodies)
    G, mag = gr.gram_exact(M, cols, wt, F, spec[0], sh, T)
    return G, mag, F, used, int(spec[0].sum())


def check_gram(path, ids, G, mag):
    """--gram against the exact matrix: per cell within (M + 8) 2^-53 (T_ij 2^-F + A_i + A_j + S) / n_used -- every term is a sum of at
    most M + 1 non-negative doubles (kmx_pca_math.hpp) --, and every row sums to zero within the row's bounds summed"""
    got_ids, got = gr.parse_gram(open(path).read())
    M = len(ids)
    assert got_ids == ids and got.shape == (M, M) and np.array_equal(got, got.T)
    u = Fraction(M + 8, 2 ** 53)
    for i in range(M):
        for j in range(M):
            err = abs(Fraction(float(got[i][j])) - G[i][j])
            print(f"G[{i}][{j}] = {got[i][j]!r}: off by {float(err):.3e}, allowed {float(u * mag[i][j]):.3e}")
            assert err <= u * mag[i][j], (i, j)
        assert abs(sum(Fraction(float(x)) for x in got[i])) <= u * sum(mag[i]), i
    return got


def check_pcs(text, evals_path, ids, G, k):
    """the printed components against numpy's on the matrix the driver wrote (the solver itself is tested without a device)"""
    got_ids, V = gr.parse_pcs(text)
    assert got_ids == ids and V.shape == (len(ids), k)
    lam = np.array([float(x) for x in open(evals_path).read().split()])
    ref = np.linalg.eigvalsh(G)[::-1]
    norm = abs(ref).max()
    assert len(lam) == len(ids) and np.abs(lam - ref).max() <= 8 * len(ids) * 2.0 ** -53 * norm
    for c in range(k):
        assert np.abs(G @ V[:, c] - lam[c] * V[:, c]).max() <= (8 * len(ids) * 2.0 ** -53 + 5e-10) * norm
        assert V[np.abs(V[:, c]).argmax(), c] > 0
    assert abs(lam[-1]) <= 8 * len(ids) * 2.0 ** -53 * norm + max(abs(G.sum(axis=1)))      # a centred matrix: the all-ones vector is in its null space


@pytest.mark.parametrize("mode", KINDS)
def test_driver_on_the_golden_samples(golden_runs, mode, tmp_path):
    """with and without --samples, --min-abund 2, --scale none, --min-rec / --max-rec, against gram_ref's exact fractions applied to the
    run's matrices; the matrix file read back with --from-gram prints the same components"""
    run = golden_runs["runs"][mode]
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, 4, 31)
    outs = ("--gram", tmp_path / "gram.tsv", "--evals", tmp_path / "ev.txt")
    G, mag, F, used, rows = restated(bodies, n, kw, rmode, None)
    assert rows > 100 and 0 < used <= rows      # every sample's own rows and shared rows; rows all three hold would be left out
    r = kmx("pca", "--run", run, *outs, "-v")
    assert r.returncode == 0, r.stderr
    assert "3 of 3 samples, 4 partitions" in r.stderr and f"F = {F}, {used} of {rows} rows used" in r.stderr
    got = check_gram(tmp_path / "gram.tsv", IDS, G, mag)
    check_pcs(r.stdout, tmp_path / "ev.txt", IDS, got, 2)
    again = kmx("pca", "--from-gram", tmp_path / "gram.tsv")
    assert again.returncode == 0 and again.stdout == r.stdout
    one = kmx("pca", "--run", run, "--pcs", 1, "--output", tmp_path / "pc1.tsv")
    assert one.returncode == 0 and one.stdout == ""
    assert [ln.split("\t")[:2] for ln in open(tmp_path / "pc1.tsv").read().splitlines()] == [ln.split("\t")[:2] for ln in r.stdout.splitlines()]
    # unscaled; one class only
    for extra, kwargs in ((("--scale", "none"), dict(scale="none")), (("--min-rec", 2), dict(min_rec=2)), (("--max-rec", 1, "--scale", "none"), dict(max_rec=1, scale="none"))):
        G2, mag2, F2, used2, _ = restated(bodies, n, kw, rmode, None, **kwargs)
        r2 = kmx("pca", "--run", run, *outs, *extra, "-v")
        assert r2.returncode == 0 and f"F = {F2}, {used2} of {rows} rows used" in r2.stderr, r2.stderr
        check_gram(tmp_path / "gram.tsv", IDS, G2, mag2)
    # a list of two samples in another order: one component
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D3\n\nD1\n")
    G3, mag3, F3, used3, _ = restated(bodies, n, kw, rmode, [2, 0])
    r3 = kmx("pca", "--run", run, *outs, "--samples", tmp_path / "s.txt", "-v")
    assert r3.returncode == 0 and f"F = {F3}, {used3} of {rows} rows used" in r3.stderr, r3.stderr
    got3 = check_gram(tmp_path / "gram.tsv", ["D3", "D1"], G3, mag3)
    check_pcs(r3.stdout, tmp_path / "ev.txt", ["D3", "D1"], got3, 1)
    if mode == "kmer:count:bin":
        G4, mag4, F4, used4, _ = restated(bodies, n, kw, rmode, None, a=2)
        assert used4 != used
        r4 = kmx("pca", "--run", run, *outs, "--min-abund", 2, "-v")
        assert r4.returncode == 0 and f"F = {F4}, {used4} of {rows} rows used" in r4.stderr, r4.stderr
        check_gram(tmp_path / "gram.tsv", IDS, G4, mag4)


def test_driver_row_runs_and_lz4(golden_runs, tmp_path):
    """a --cpr run gives what the plain run gives; --batch-mb 1 cuts every partition of a hand-made run (100 count columns, 3000 rows a
    partition) into runs of rows"""
    run = golden_runs["runs"]["kmer:count:bin"]
    r = kmx(*golden_runs["base"], "--file", golden_runs["dir"] / "in.fof", "--run-dir", tmp_path / "lz", "--mode", "kmer:count:bin", "--cpr")
    assert r.returncode == 0, r.stderr
    plain = kmx("pca", "--run", run, "--gram", tmp_path / "g1.tsv")
    lz = kmx("pca", "--run", tmp_path / "lz", "--gram", tmp_path / "g2.tsv")
    assert plain.returncode == 0 and lz.returncode == 0, lz.stderr
    assert lz.stdout == plain.stdout and open(tmp_path / "g1.tsv").read() == open(tmp_path / "g2.tsv").read()
    # 1 MB: two runs in flight, 512 KB each -- rows of 8 + 4 * 100 bytes + 25: 1210 rows a run, 3000 rows a partition
    ids = [f"S{j}" for j in range(100)]
    bodies = [pr.shaped_body(140 + p, 3000, 100, 1, COUNT, "uniform") for p in range(3)]
    root = dr.write_run(tmp_path / "wide", "hash:count:bin", 31, ids, bodies, window=16)
    G, mag, F, used, rows = restated(bodies, 100, 1, COUNT, None)
    r = kmx("pca", "--run", root, "--gram", tmp_path / "wide.tsv", "--batch-mb", 1, "-v")
    assert r.returncode == 0, r.stderr
    assert "runs of 1210 rows" in r.stderr and f"F = {F}, {used} of {rows} rows used" in r.stderr
    check_gram(tmp_path / "wide.tsv", ids, G, mag)
    assert len(r.stdout.splitlines()) == 101 and r.stdout.splitlines()[0].split("\t")[-1] == "PC10"


def test_driver_on_two_devices(golden_runs, tmp_path):
    """--gpus 2: partition p on shard p mod 2, the shards' tables summed on the host -- the same matrix, digit for digit"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    run = golden_runs["runs"]["kmer:pa:bin"]
    a = kmx("pca", "--run", run, "--gram", tmp_path / "g1.tsv")
    b = kmx("pca", "--run", run, "--gram", tmp_path / "g2.tsv", "--gpus", 2)
    assert a.returncode == 0 and b.returncode == 0, b.stderr
    assert b.stdout == a.stdout and open(tmp_path / "g1.tsv").read() == open(tmp_path / "g2.tsv").read()
