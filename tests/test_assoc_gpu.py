"""`kmx assoc` on the MI355X against tests/assoc_ref.py: the C ABI through kmtricks_amd.lib on the bodies of assoc_ref.gpu_cases() -- kept
rows, rec and s0 exactly, stat and beta bit for bit, the kept body byte for byte --, the body at odd addresses and device-resident, the
limits, the launch shapes the two knobs of assoc.hip force, and the driver on a run of eight samples cut from the golden ones.  Run with
-m gpu."""
import ctypes as C
import math, os, re, struct, subprocess

import numpy as np
import pytest

import assoc_ref as ar
import dist_ref as dr
import pan_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = ar.MODE_COUNT, ar.MODE_PA
U32, INF = ar.U32, ar.INF


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, what):
    """kept rows, rec, s0 exactly; stat and beta bit for bit (only correctly rounded + - * / and exact conversions occur); the records in
    file order; the kept body byte for byte"""
    recs, body = exp
    assert out.recs.dtype == ar.REC and len(out.recs) == len(recs), (what, len(out.recs), len(recs))
    assert np.array_equal(out.recs["row"], recs["row"]), what
    assert (np.diff(out.recs["row"].astype(np.int64)) > 0).all(), what
    assert np.array_equal(out.recs["rec"], recs["rec"]) and np.array_equal(out.recs["s0"], recs["s0"]), what
    for f in ("stat", "beta"):
        d = out.recs[f].view(np.uint64) != recs[f].view(np.uint64)
        assert not d.any(), f"{what}: {f} differs in {int(d.sum())} records, first at row {out.recs['row'][d][:3]}: {out.recs[f][d][:3]!r} for {recs[f][d][:3]!r}"
    assert out.body == body, what


def run_case(ctx, c):
    out = ctx.assoc(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, **c.params())
    same(out, c.expected, c.name)
    assert out.algo_bytes == ar.algo_bytes(c.n_rows, c.n_cols, c.key_words, c.mode, c.n_vec, len(c.expected[0]))
    return out


def test_header_example(ctx):
    from test_assoc_cpu import example_body, EX_VECS, EX_ALL
    for mode in (COUNT, PA):
        out = ctx.assoc(example_body(mode), 4, 4, 1, mode, EX_VECS, 2, 3.0, 0.25, 1.0)
        assert [(int(r["rec"]), int(r["s0"]), float(r["stat"]), float(r["beta"]), int(r["row"])) for r in out.recs] == [EX_ALL[0] + (0,), EX_ALL[3] + (3,)]
        rb = dr.row_bytes(1, 4, mode)
        assert out.body == example_body(mode).reshape(4, rb)[[0, 3]].tobytes()
        every = ctx.assoc(example_body(mode), 4, 4, 1, mode, EX_VECS, 2, 3.0, 0.25, 0.0)
        assert [(int(r["rec"]), int(r["s0"]), float(r["stat"]), float(r["beta"])) for r in every.recs] == EX_ALL


@pytest.mark.parametrize("name", [c.name for c in ar.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of a byte, of a block of 64 counts and of 64 payload bytes; rows on both sides of a wave's group of 64 and of a
    placement tile of 256; V on both sides of every step of the kernel's vector count (VP_STEPS) and past the 8 (COUNT) and 4 (PA) vectors
    of one walk; lists of every kind; entries of +-2^30 everywhere (a 32-bit partial sum wraps from the second column on); all-zero rows,
    all-ones rows with every padding bit set, counts of 2^32 - 1 at min_abund 1, 2, 2^32 - 1; thresholds 0, +inf and the median statistic
    (rows sit exactly on it); windows, an empty one among them; vmin 0 and above every v; key widths 1 ... 4"""
    run_case(ctx, ar.case(name))


ODD = [c.name for c in ar.gpu_cases() if c.name.endswith("-cut")][::3] + [c.name for c in ar.gpu_cases() if c.name.endswith("-block")]


@pytest.mark.parametrize("name", ODD)
def test_body_at_an_odd_host_address_and_device_resident(ctx, name):
    """the body handed in at an odd host address, and through _dev from every device alignment: the same result"""
    import torch
    c = ar.case(name)
    buf = np.zeros(len(c.body) + 9, np.uint8)
    for shift in (1, 3):
        view = buf[shift:shift + len(c.body)]
        view[:] = c.body
        assert view.ctypes.data % 2 == 1
        same(ctx.assoc(view, c.n_rows, c.n_cols, c.key_words, c.mode, **c.params()), c.expected, (name, "host", shift))
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 5):
        d = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        d[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        out = ctx.assoc_dev(d.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, **c.params())
        same(out, c.expected, (name, "dev", shift))


def test_result_left_on_the_device(ctx):
    """keep=True: the kept rows and records stay in HBM; another call reads them as its body"""
    c = ar.case(next(x.name for x in ar.gpu_cases() if x.name.endswith("-cut") and x.mode == COUNT and len(x.expected[0]) > 10))
    r = ctx.assoc(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, keep=True, **c.params())
    try:
        n = r.rows()
        assert n == len(c.expected[0]) and r.row_bytes() == dr.row_bytes(c.key_words, c.n_cols, c.mode) and r.body_bytes() == len(c.expected[1])
        assert r.recs_dev()
        again = ctx.assoc_dev(r.body_dev(), n, c.n_cols, c.key_words, c.mode, **c.params())      # the kept rows are kept again
        assert again.body == c.expected[1] and again.recs["stat"].tobytes() == c.expected[0]["stat"].tobytes()
        assert list(again.recs["row"]) == list(range(n))
    finally:
        r.free()


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    big = np.full((4, 32), 2 ** 30, np.int32)

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, a=1, flags=0, n_rows=0, vecs=big, V=2, F=30, gain=1.0, vmin=0.0, thr=0.0):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        M = (N if cc is None else len(cc)) if M is None else M
        for fn in (lib._lib.kmx_assoc_host, lib._lib.kmx_assoc_dev):
            t = lib.KmxAssocTask(kw, mode, N, M, None, n_rows, None if cc is None else cc.ctypes.data, None if vecs is None else vecs.ctypes.data, V, F, a, flags,
                                 gain, vmin, thr, 0, U32)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, a, flags, n_rows, V, F, gain, vmin, thr)

    OK, INVAL, UNSUP = 0, -2, -5
    call(INVAL, N=0, cols=None); call(INVAL, M=0)
    call(INVAL, N=2, cols=(0, 1, 0))                               # n_use > n_cols
    call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4))       # an index at N; a duplicate
    call(INVAL, cols=None, M=8)                                    # the identity with M != N
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, mode=7)
    call(INVAL, a=0); call(INVAL, a=0, mode=PA); call(INVAL, a=2, mode=PA)
    call(INVAL, V=0); call(INVAL, V=33)
    call(INVAL, vecs=None)
    call(INVAL, F=63)
    call(INVAL, gain=0.0); call(INVAL, gain=-1.0); call(INVAL, gain=INF); call(INVAL, gain=float("nan"))
    call(INVAL, vmin=-1e-300); call(INVAL, vmin=float("nan"))
    call(INVAL, thr=float("nan")); call(INVAL, thr=-0.5)
    call(INVAL, flags=1); call(INVAL, flags=0x80000000)
    # a vector whose magnitudes sum to 2^53: 2^22 listed samples of 2^31 each (the second vector; the first stays below)
    M = 2 ** 22
    v = np.zeros((M, 2), np.int32)
    v[:, 0] = 2 ** 30
    v[:, 1] = -2 ** 31
    call(INVAL, N=M, cols=None, vecs=v, mode=PA)
    v[0, 1] = -2 ** 31 + 1                                         # one below: taken (no rows: nothing runs)
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode); call(UNSUP, mode=mode, kw=0)
    call(UNSUP, N=2 ** 30, cols=None)                              # a row of 8 + 2^32 bytes (refused before the vectors are looked at)
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32 - 255, mode=PA)
    # what is valid is taken: no rows yield nothing; F = 62, threshold +inf
    for vecs, N, cols, mode in ((big, 9, np.array([4, 2, 1], np.uint32), COUNT), (v, M, None, PA)):
        t = lib.KmxAssocTask(1, mode, N, len(vecs) if cols is None else len(cols), None, 0, None if cols is None else cols.ctypes.data, vecs.ctypes.data, 2, 62, 1, 0,
                             1.0, 0.0, INF, 0, U32)
        res = C.c_void_p()
        assert lib._lib.kmx_assoc_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
        assert lib._lib.kmx_assoc_result_rows(res) == 0 and lib._lib.kmx_assoc_result_body_bytes(res) == 0
        assert lib._lib.kmx_assoc_result_copy_body(res, None, 0) == OK and lib._lib.kmx_assoc_result_copy_recs(res, None, 0) == OK
        assert lib._lib.kmx_assoc_result_algo_bytes(res) == 4 * N * 2
        lib._lib.kmx_assoc_result_free(res)
    # the context stays usable
    run_case(ctx, ar.case(next(x.name for x in ar.gpu_cases() if x.name.startswith("c-7-"))))


# ---- the launch shapes KMX_ASSOC_CUS and KMX_ASSOC_GRID force --------------------------------------------------------------------
def launch_shape(n_rows, cus, grid_cap):
    """the launcher's formulas (assoc.hip, assoc_queue) -> trips of each kernel's stride loop"""
    groups = (n_rows + 63) // 64
    cap = min(1 << 18, grid_cap)
    score_grid = min(groups, min(cus * 32, cap))
    tiles = (n_rows + 255) // 256
    place_grid = min(tiles, cap)
    return dict(score=-(-groups // score_grid), place=-(-tiles // place_grid))


@pytest.mark.parametrize("mode,N,rows,V,kind", [(COUNT, 130, 3000, 3, "subset"), (PA, 1100, 3000, 2, "none"), (COUNT, 40, 5001, 17, "second"), (PA, 130, 5001, 9, "subset")])
def test_launch_shapes(ctx, mode, N, rows, V, kind, monkeypatch):
    """KMX_ASSOC_CUS=1 and KMX_ASSOC_GRID=3 (read per call): several trips of each stride loop; each shape against the reference and,
    byte for byte, against the same call with the knobs unset"""
    import torch
    kw = 1 + N % 4
    body = pr.shaped_body(3234 + N, rows, N, kw, mode, "uniform")
    cols = ar.make_cols(kind, N, 9)
    M = N if cols is None else len(cols)
    vecs = ar.make_vecs("random", M, V, 77)
    a = ar.assoc_rows_np(body, N, kw, mode, vecs, 30, 2.5, 2.0 ** -10, cols)
    thr = float(np.sort(a["stat"])[len(a) // 2])
    exp = ar.assoc_expected_np(body, N, kw, mode, vecs, 30, 2.5, 2.0 ** -10, thr, cols, 1, 1, M - 1)
    assert 0 < len(exp[0]) < rows
    args = dict(vecs=vecs, frac_bits=30, gain=2.5, vmin=2.0 ** -10, threshold=thr, cols=cols, min_rec=1, max_rec=M - 1)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.delenv("KMX_ASSOC_CUS", raising=False); monkeypatch.delenv("KMX_ASSOC_GRID", raising=False)
    base = ctx.assoc(body, rows, N, kw, mode, **args)
    same(base, exp, "knobs unset")
    for env in (dict(KMX_ASSOC_CUS="1"), dict(KMX_ASSOC_GRID="3"), dict(KMX_ASSOC_CUS="1", KMX_ASSOC_GRID="3")):
        shape = launch_shape(rows, 1 if "KMX_ASSOC_CUS" in env else n_cu, 3 if "KMX_ASSOC_GRID" in env else 1 << 18)
        assert shape["score"] > 1, (env, shape)
        if "KMX_ASSOC_GRID" in env:
            assert shape["place"] > 1, (env, shape)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.assoc(body, rows, N, kw, mode, **args)
        for k in env:
            monkeypatch.delenv(k)
        same(out, exp, env)
        assert out.body == base.body and out.recs.tobytes() == base.recs.tobytes()


# ---- the driver on eight samples cut from the golden ones ----------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


IDS = [f"E{i + 1}" for i in range(8)]
PHENO = [2.0, 1.8, 2.2, 1.5, 0.1, -0.2, 0.3, 0.0]
MODES = ("kmer:count:bin", "hash:pa:bin")


def bloom(mode):
    return ("--bloom-size", 1000000) if mode.startswith("hash:") else ()


@pytest.fixture(scope="module")
def eight(tmp_path_factory):
    """`kmx pipeline --hard-min 1`, 4 partitions, over eight samples made of slices of the two golden samples' four reads: the first
    four hold the first read (the phenotype follows it), the rest hold other parts.  kmer:count:bin plain; hash:pa:bin plain (the
    reference reads it) and with --cpr (the driver reads it)"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxassoc")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    one, two = (open(os.path.join(GD, f"{i}.fasta")).read().split("\n") for i in (1, 2))
    A, B, Cc, D = one[1], one[3], two[1], two[3]
    parts = [[A, Cc[:60], A], [A, D[20:]], [A, B[:70]], [A[:80], Cc[30:], B[40:]], [B, Cc], [D, B[10:80]], [Cc[:70], D[:60]], [D[30:], Cc[20:90]]]      # (E1 holds A twice: counts of 2)
    for i, reads in enumerate(parts):
        with open(d / f"{i + 1}.fasta", "w") as f:
            f.write("".join(f">r{j}\n{r}\n" for j, r in enumerate(reads)))
    with open(d / "in.fof", "w") as f:
        f.write("".join(f"{IDS[i]} : {d}/{i + 1}.fasta\n" for i in range(8)))
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--soft-min", 1, "--recurrence-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    runs = {}
    for mode in MODES:
        run = d / mode.replace(":", "_")
        r = kmx(*base, "--run-dir", run, "--mode", mode, *bloom(mode))
        assert r.returncode == 0, r.stderr
        runs[mode] = dict(plain=run, use=run)
    lz = d / "hash_pa_lz4"
    r = kmx(*base, "--run-dir", lz, "--mode", "hash:pa:bin", "--cpr", *bloom("hash:pa:bin"))
    assert r.returncode == 0, r.stderr
    assert open(lz / "matrices" / "matrix_0.pa_hash", "rb").read()[12] == 1      # the header says: an lz4 body
    runs["hash:pa:bin"]["use"] = lz
    # the covariates: the first two principal components of the eight samples
    r = kmx("pca", "--run", runs["kmer:count:bin"]["plain"], "--pcs", 2, "--output", d / "pcs.tsv")
    assert r.returncode == 0, r.stderr
    return dict(dir=d, runs=runs, covar=d / "pcs.tsv")


def parse_design(path):
    lines = open(path).read().splitlines()
    head = dict(ln.split("\t") for ln in lines[1:7])
    cells = [ln.split("\t") for ln in lines[8:]]
    return dict(F=int(head["F"]), M=int(head["M"]), q=int(head["q"]), gain=float(head["gain"]), vmin=float(head["vmin"]), ymax=float(head["ymax"]),
                ids=[c[0] for c in cells], cols=[int(c[1]) for c in cells], vecs=np.array([[int(x) for x in c[2:]] for c in cells], np.int64))


def kmer_string(key, k):
    w = np.frombuffer(key, "<u8")
    return "".join("ACTG"[(int(w[(k - 1 - i) >> 5]) >> (((k - 1 - i) & 31) * 2)) & 3] for i in range(k))


def p_of(stat):
    return math.erfc(math.sqrt(stat / 2.0))


def threshold_of(p):
    lo, hi = 0.0, 2000.0
    if p_of(lo) <= p:
        return lo
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if p_of(mid) <= p:
            hi = mid
        else:
            lo = mid
    return hi


RATIOS = []


def check_driver(eight, mode, listed, covar, alpha, tmp_path, extra=()):
    """one run of the driver against the restatement fed with the --design integers, and every kept row's statistic against float64
    least squares on the unquantised design.  -> the kept lines"""
    g = eight["runs"][mode]
    bodies, n, kw, rmode = dr.read_run_bodies(g["plain"], mode, 4, 31)
    assert n == 8
    ph = tmp_path / "ph.txt"
    with open(ph, "w") as f:
        f.write("".join(f"{IDS[i]}\t{PHENO[i]!r}\n" for i in reversed(listed)))      # (any order: the design is in fof order)
    args = ["assoc", "--run", g["use"], "--pheno", ph, "--design", tmp_path / "des.tsv", "--correction", "none", "--alpha", alpha, "-v", *extra]
    if covar:
        args += ["--covar", eight["covar"], "--pcs", 2]
    r = kmx(*args)
    assert r.returncode == 0, r.stderr
    D = parse_design(tmp_path / "des.tsv")
    M, q = len(listed), 3 if covar else 1
    assert (D["F"], D["M"], D["q"], D["ids"], D["cols"]) == (30, M, q, [IDS[i] for i in listed], list(listed))
    thr = float(re.search(r"statistic >= (\S+)", r.stderr).group(1))
    assert abs(thr - threshold_of(float(alpha))) <= 1e-9 * thr
    cols = None if M == 8 else np.array(listed, np.uint32)
    # the unquantised design, by numpy
    y = np.array([PHENO[i] for i in listed])
    Cm = np.ones((M, 1))
    if covar:
        cells = [ln.split("\t") for ln in open(eight["covar"]).read().splitlines()[1:]]
        pcs = {c[0]: [float(x) for x in c[1:3]] for c in cells}
        Cm = np.concatenate([Cm, np.array([pcs[IDS[i]] for i in listed])], axis=1)
    Qn = np.linalg.qr(Cm)[0]
    yt = y - Cm @ np.linalg.lstsq(Cm, y, rcond=None)[0]
    d31, B = 2.0 ** -31, ar_v_bound(M, q)
    want, tested = [], 0
    for body in bodies:
        a = ar.assoc_rows_np(body, 8, kw, rmode, D["vecs"], 30, D["gain"], D["vmin"], cols)
        inside = (a["rec"] >= 1) & (a["rec"] <= M - 1)
        tested += int(inside.sum())
        X = ar.presence(body, 8, kw, rmode, cols).astype(np.float64)
        rb = dr.row_bytes(kw, 8, rmode)
        rows = np.frombuffer(dr.as_bytes(body), np.uint8).reshape(-1, rb)
        for i in np.flatnonzero(inside & (a["stat"] >= thr)):
            key = kmer_string(rows[i, :8 * kw].tobytes(), 31) if mode.startswith("kmer") else str(int(np.frombuffer(rows[i, :8].tobytes(), "<u8")[0]))
            st, be, rec = float(a["stat"][i]), float(a["beta"][i]), int(a["rec"][i])
            line = key + "\t%.6e\t%.6f\t%.6g\t%u" % (p_of(st), st, be * D["ymax"], rec)
            if "--counts" in extra:
                pay = dr.split_payload(body, 8, kw, rmode)[i]
                line += "".join("\t%d" % int(v) for v in pay)
            want.append(line)
            # float64 least squares on the unquantised design: (M - q) r^2 of the partial correlation
            x = X[i]
            u, v = x @ yt, x @ x - ((Qn.T @ x) ** 2).sum()
            exact = (M - q) * u * u / ((yt @ yt) * v)
            # the quantisation bound of vmin, propagated: u (in units of ymax) is off by at most rec 2^-31, the sum of squares of vector 0 by
            # at most M (2^-30 + 2^-62), v by at most B -- the statistic lies between the two ends of the interval
            uq, syy = abs(u) / D["ymax"], (yt @ yt) / D["ymax"] ** 2
            du, ds = rec * d31, M * (2 * d31 + d31 * d31)
            hi = (M - q) * (uq + du) ** 2 / ((syy - ds) * (v - B))
            lo = (M - q) * max(uq - du, 0.0) ** 2 / ((syy + ds) * (v + B))
            bound = max(hi - exact, exact - lo) + 1e-12 * exact
            assert v > B and abs(st - exact) <= bound, (key, st, exact, bound)
            RATIOS.append(abs(st - exact) / bound)
    assert f"{tested} of {sum(len(b) // dr.row_bytes(kw, 8, rmode) for b in bodies)} rows tested" in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    head = ("kmer" if mode.startswith("kmer") else "hash") + "\tpvalue\tstat\tbeta\trec" + ("".join("\t" + s for s in IDS) if "--counts" in extra else "")
    assert lines[0] == head
    assert lines[1:] == want      # kept keys and their order exactly; p, stat, beta as printed
    return lines[1:]


def ar_v_bound(M, q):
    d = 2.0 ** -31
    return q * (2 * M * math.sqrt(M) * d + M * M * d * d) + (q + 2) * M * 2.0 ** -50


@pytest.mark.parametrize("mode", MODES)
def test_driver_on_eight_samples(eight, mode, tmp_path):
    """with and without --covar (the covariates `kmx pca --pcs 2` wrote for the same run); every sample listed, and seven of the eight;
    the hash:pa:bin run is read from its --cpr form"""
    every = list(range(8))
    kept = check_driver(eight, mode, every, False, "0.05", tmp_path, extra=("--counts",) if mode == "kmer:count:bin" else ())
    assert len(kept) >= 1      # the phenotype follows the first read: its rows are significant without a correction
    check_driver(eight, mode, every, True, "0.5", tmp_path)
    seven = [0, 1, 2, 3, 4, 6, 7]
    assert len(check_driver(eight, mode, seven, False, "0.05", tmp_path)) >= 1
    check_driver(eight, mode, seven, True, "0.5", tmp_path)
    print(f"[assoc] {mode}: largest |stat - least squares| / bound over {len(RATIOS)} kept rows: {max(RATIOS):.3e}")


def test_driver_bonferroni_rows_and_output_file(eight, tmp_path):
    """the default correction divides alpha by the rows inside the window; --output writes the file and nothing to standard output;
    --batch-mb 1 on a hand-made wide run cuts every partition into runs of rows: the same lines as one run a partition"""
    g = eight["runs"]["kmer:count:bin"]
    ph = tmp_path / "ph.txt"
    with open(ph, "w") as f:
        f.write("".join(f"{IDS[i]} {PHENO[i]!r}\n" for i in range(8)))
    r = kmx("assoc", "--run", g["use"], "--pheno", ph, "-v", "--output", tmp_path / "o.tsv")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    m = re.search(r"(\d+) of (\d+) rows tested \(recurrence 1 \.\.\. 7\), p <= (\S+), statistic >= (\S+)", r.stderr)
    assert m and abs(float(m.group(3)) - 0.05 / int(m.group(1))) <= 1e-6 * float(m.group(3))
    assert abs(float(m.group(4)) - threshold_of(0.05 / int(m.group(1)))) <= 1e-9 * float(m.group(4))
    assert open(tmp_path / "o.tsv").read().splitlines()[0] == "kmer\tpvalue\tstat\tbeta\trec"
    ids = [f"S{j}" for j in range(100)]
    bodies = [pr.shaped_body(240 + p, 3000, 100, 1, COUNT, "uniform") for p in range(3)]
    root = dr.write_run(tmp_path / "wide", "hash:count:bin", 31, ids, bodies, window=16)
    rng = np.random.default_rng(5)
    with open(tmp_path / "wide.ph", "w") as f:
        f.write("".join(f"S{j} {float(v)!r}\n" for j, v in enumerate(rng.normal(size=100)) if j % 7))
    one = kmx("assoc", "--run", root, "--pheno", tmp_path / "wide.ph", "--correction", "none", "--alpha", "0.01")
    cut = kmx("assoc", "--run", root, "--pheno", tmp_path / "wide.ph", "--correction", "none", "--alpha", "0.01", "--batch-mb", 1, "-v")
    assert one.returncode == 0 and cut.returncode == 0, cut.stderr
    mt = re.search(r"runs of (\d+) rows", cut.stderr)
    assert mt and int(mt.group(1)) < 3000
    assert cut.stdout == one.stdout and 10 < len(one.stdout.splitlines()) < 9000


def test_driver_on_two_devices(eight, tmp_path):
    """--gpus 2: partition p on shard p mod 2 -- the same text"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    g = eight["runs"]["hash:pa:bin"]
    ph = tmp_path / "ph.txt"
    with open(ph, "w") as f:
        f.write("".join(f"{IDS[i]} {PHENO[i]!r}\n" for i in range(8)))
    a = kmx("assoc", "--run", g["use"], "--pheno", ph, "--correction", "none")
    b = kmx("assoc", "--run", g["use"], "--pheno", ph, "--correction", "none", "--gpus", 2)
    assert a.returncode == 0 and b.returncode == 0, b.stderr
    assert b.stdout == a.stdout and len(a.stdout.splitlines()) > 1
