"""`kmx dist` on the MI355X against tests/dist_ref.py: the C ABI through kmtricks_amd.lib on synthetic bodies -- exact equality of the
inter and mins tables with the numpy road of the restatement --, and the driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, re, shutil, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA, BF = dr.MODE_COUNT, dr.MODE_PA, dr.MODE_BF
KW = {COUNT: 1, PA: 1, BF: 0}
# rows of the shortest run a workgroup of k_dist_pairs takes at a time: DP_RUN_MIN = 64 words of 64 rows (kmtricks_amd/csrc/dist.hip);
# a body of one block pair (N <= 64) longer than that is cut into runs
PAIRS_RUN_ROWS = 64 * 64


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, what):
    ei, em = exp
    bad = np.argwhere(out.inter != ei)
    assert not len(bad), f"{what}: inter differs in {len(bad)} cells, first (i, j) {bad[:4].tolist()}: got {[int(out.inter[tuple(b)]) for b in bad[:4]]}, expected {[int(ei[tuple(b)]) for b in bad[:4]]}"
    if em is None:
        assert out.mins is None
    else:
        bad = np.argwhere(out.mins != em)
        assert not len(bad), f"{what}: mins differ in {len(bad)} cells, first (i, j) {bad[:4].tolist()}: got {[int(out.mins[tuple(b)]) for b in bad[:4]]}, expected {[int(em[tuple(b)]) for b in bad[:4]]}"


def check(ctx, body, N, kw, mode, what=""):
    """host road, with mins for count rows; the table is symmetric and its diagonal is the column sums"""
    exp = dr.dist_expected_np(body, N, kw, mode, mins=mode == COUNT)
    out = ctx.dist(body, None, N, kw, mode, mins=mode == COUNT)
    same(out, exp, what)
    assert np.array_equal(out.inter, out.inter.T)
    assert np.array_equal(np.diag(out.inter), (dr.split_payload(body, N, kw, mode) != 0).sum(axis=0).astype(np.uint64))
    return out, exp


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
@pytest.mark.parametrize("N", [1, 7, 8, 9, 63, 64, 65, 100, 128, 129, 1000])
def test_columns(ctx, N, mode):
    """both sides of the byte, the 64-sample block and the 512-column tile; every padding bit of every PA / BF row is 1; rows of
    8 + ceil(N / 8) bytes start at every alignment"""
    rows = 150 if N < 1000 else 131
    body = dr.make_body(10 * N + mode, rows, N, KW[mode], mode, 0.3, pad_ones=True, maxed=0.02)
    if mode != COUNT and N % 8:
        assert (body.reshape(rows, -1)[:, -1] >> (N % 8)).min() == (0xFF >> (N % 8))
    out, exp = check(ctx, body, N, KW[mode], mode, f"N={N} mode={mode}")
    assert exp[0].any()


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_many_samples(ctx, mode):
    """2500 samples x 70 rows: 40 blocks of samples, 820 block pairs"""
    N = 2500
    body = dr.make_body(77 + mode, 70, N, 1, mode, 0.1, pad_ones=True)
    check(ctx, body, N, 1, mode, f"N={N}")


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, PAIRS_RUN_ROWS - 1, PAIRS_RUN_ROWS, PAIRS_RUN_ROWS + 1, 3 * PAIRS_RUN_ROWS + 5])
def test_rows(ctx, rows, mode):
    """both sides of a slab word (64 rows), of a workgroup's run and of several runs; no rows at all"""
    N = 9 if mode == COUNT else 70
    body = dr.make_body(rows + mode, rows, N, KW[mode], mode, 0.4, pad_ones=True)
    out, exp = check(ctx, body, N, KW[mode], mode, f"rows={rows} mode={mode}")
    assert bool(exp[0].any()) == (rows > 0)


@pytest.mark.parametrize("mode,kw", [(COUNT, 1), (COUNT, 2), (COUNT, 3), (COUNT, 4), (PA, 1), (PA, 2), (PA, 3), (PA, 4), (BF, 0)])
def test_key_words(ctx, mode, kw):
    """keys of every width are stepped over, never read (they are random bytes)"""
    body = dr.make_body(kw, 200, 13, kw, mode, 0.5)
    check(ctx, body, 13, kw, mode, f"kw={kw} mode={mode}")


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
def test_extreme_bodies(ctx, mode):
    """a body of zeros; a body of ones (every key byte, count byte and padding bit); five rows of 2^32 - 1: mins pass 2^34"""
    N, rows = 67, 130
    rb = dr.row_bytes(KW[mode], N, mode)
    out, _ = check(ctx, np.zeros(rows * rb, np.uint8), N, KW[mode], mode, "zeros")
    assert not out.inter.any()
    out, _ = check(ctx, np.full(rows * rb, 0xFF, np.uint8), N, KW[mode], mode, "ones")
    assert (out.inter == rows).all()
    if mode == COUNT:
        assert (out.mins == rows * 0xFFFFFFFF).all()
        out, _ = check(ctx, np.full(5 * rb, 0xFF, np.uint8), N, 1, COUNT, "five rows of 2^32 - 1")
        assert (out.mins == 5 * 0xFFFFFFFF).all() and int(out.mins[3, 60]) > 2 ** 34


@pytest.fixture(scope="module")
def bodies():
    """one body a mode, N = 100, 5000 rows, and what it gives: worked out once"""
    out = {}
    for mode in (COUNT, PA, BF):
        body = dr.make_body(40 + mode, 5000, 100, KW[mode], mode, 0.3, maxed=0.01)
        out[mode] = (body, dr.dist_expected_np(body, 100, KW[mode], mode, mins=mode == COUNT))
    return out


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
def test_device_resident_and_odd_address(ctx, bodies, mode):
    """host and device-resident inputs give the same tables; a body that starts at an odd device address; the algorithmic bytes"""
    import torch
    body, exp = bodies[mode]
    N, kw, rows = 100, KW[mode], 5000
    rb = dr.row_bytes(kw, N, mode)
    host = ctx.dist(body, None, N, kw, mode, mins=mode == COUNT)
    same(host, exp, "host")
    dev = torch.device("cuda:0")
    for shift in (0, 1, 3):
        buf = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
        buf[shift:shift + len(body)] = torch.from_numpy(body.copy()).to(dev)
        torch.cuda.synchronize()
        ptr = buf.data_ptr() + shift
        assert ptr % 2 == (shift % 2)
        out = ctx.dist_dev(ptr, rows, N, kw, mode, mins=mode == COUNT)
        same(out, exp, f"device-resident, address + {shift}")
        slab = 2 * (128 // 8) * ((rows + 63) // 64 * 64)
        want = rows * rb + slab + 8 * N * N + ((4 * N * rows + 8 * N * N) if mode == COUNT else 0)
        assert out.algo_bytes == want == host.algo_bytes


@pytest.mark.parametrize("mode", [COUNT, PA, BF])
def test_series_add_up(ctx, bodies, mode):
    """three calls over the thirds of a body into one given table equal one call over the whole; a second series into the table that
    already holds numbers adds to them; the order of the calls does not matter"""
    import torch
    body, exp = bodies[mode]
    N, kw, rows = 100, KW[mode], 5000
    rb = dr.row_bytes(kw, N, mode)
    dev = torch.device("cuda:0")
    t_inter = torch.zeros(N * N, dtype=torch.int64, device=dev)
    t_mins = torch.zeros(N * N, dtype=torch.int64, device=dev) if mode == COUNT else None
    torch.cuda.synchronize()
    cuts = [0, 1667, 3334, rows]
    table = lambda t: t.cpu().numpy().view(np.uint64).reshape(N, N)
    for series, order in ((1, (0, 1, 2)), (2, (2, 0, 1))):
        for i in order:
            part = body[cuts[i] * rb:cuts[i + 1] * rb]
            out = ctx.dist(part, None, N, kw, mode, inter_dev=t_inter.data_ptr(), mins_dev=t_mins.data_ptr() if mode == COUNT else None)
        torch.cuda.synchronize()
        assert np.array_equal(table(t_inter), series * exp[0]), f"series {series}"
        assert np.array_equal(out.inter, series * exp[0])      # the result hands back the table as it stands
        if mode == COUNT:
            assert np.array_equal(table(t_mins), series * exp[1]) and np.array_equal(out.mins, series * exp[1])
    # a call of no rows adds nothing
    ctx.dist(b"", 0, N, kw, mode, inter_dev=t_inter.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(table(t_inter), 2 * exp[0])


def test_kept_result_and_mins_off(ctx, bodies):
    from kmtricks_amd import lib
    body, exp = bodies[COUNT]
    r = ctx.dist(body, None, 100, 1, COUNT, keep=True)
    try:
        assert r.inter_dev() and r.mins_dev() is None
        buf = np.zeros(100 * 100, np.uint64)
        assert lib._lib.kmx_dist_result_copy_mins(r._h, buf.ctypes.data, buf.size) == -2      # KMX_E_INVAL without want_mins
        assert np.array_equal(r.output().inter, exp[0]) and r.output().mins is None
    finally:
        r.free()


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    body = dr.make_body(1, 4, 3, 1, COUNT)

    def call(code, kw=1, mode=COUNT, N=3, want=0, inter=None, mins=None, rows=body.ctypes.data, n_rows=0):
        for fn in (lib._lib.kmx_dist_host, lib._lib.kmx_dist_dev):
            t = lib.KmxDistTask(kw, mode, N, want, rows, n_rows, inter, mins)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, want)

    INVAL, UNSUP = -2, -5
    call(INVAL, N=0)
    call(INVAL, mode=7)
    call(INVAL, kw=5)
    call(INVAL, kw=0, mode=COUNT); call(INVAL, kw=0, mode=PA)
    call(INVAL, kw=1, mode=BF)
    call(INVAL, mode=PA, want=1); call(INVAL, kw=0, mode=BF, want=1)
    call(INVAL, mode=PA, mins=0x1000); call(INVAL, kw=0, mode=BF, mins=0x1000)
    call(INVAL, mode=COUNT, want=0, mins=0x1000)
    call(UNSUP, N=32769); call(UNSUP, N=32769, mode=PA)
    call(UNSUP, N=2 ** 30)                                   # a row of 8 + 2^32 bytes
    call(UNSUP, kw=0, mode=lib.MODE_BFC); call(UNSUP, kw=0, mode=lib.MODE_BFT); call(UNSUP, kw=1, mode=lib.MODE_BFC)
    # and the calls that are inside every limit run
    out = ctx.dist(body, 4, 3, 1, COUNT, mins=True)
    same(out, dr.dist_expected_np(body, 3, 1, COUNT, mins=True), "inside the limits")
    # 32768 samples are inside the limit: a call of no rows into a table of the caller's touches neither (no 8 GiB table is made)
    import torch
    t = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    r = ctx.dist_dev(None, 0, 32768, 0, BF, inter_dev=t.data_ptr(), keep=True)
    try:
        r.wait()
        assert r.inter_dev() == t.data_ptr()
    finally:
        r.free()


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def expected_of(run, mode, n_parts=4, k=31):
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, n_parts, k)
    inter, mins = np.zeros((n, n), np.uint64), np.zeros((n, n), np.uint64)
    for b in bodies:
        i, m = dr.dist_expected_np(b, n, kw, rmode, mins=rmode == COUNT, blas=True)
        inter += i
        if m is not None:
            mins += m
    return inter, (mins if rmode == COUNT else None), sum(len(b) for b in bodies)


def bloom(mode):
    return ("--bloom-size", 1000000) if mode.startswith("hash:") else ()


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples in the five modes `kmx dist` reads, with the fixture's repartition table"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxdist")
    t = repart_table()
    with open(d / "fixture.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(t), 1)); f.write(t.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(d / "in.fof", "w") as f:
        f.write(f"D1 : {GD}/1.fasta\nD2 : {GD}/2.fasta\n")
    base = ["pipeline", "--file", d / "in.fof", "--kmer-size", 31, "--hard-min", 1, "--nb-partitions", 4, "--repart-file", d / "fixture.minimRepart"]
    runs = {}
    for mode in dr.KINDS:
        run = d / mode.replace(":", "_")
        r = kmx(*base, "--run-dir", run, "--mode", mode, *bloom(mode))
        assert r.returncode == 0, r.stderr
        runs[mode] = dict(run=run, exp=expected_of(run, mode))
    return dict(dir=d, base=base, runs=runs)


@pytest.mark.parametrize("mode", list(dr.KINDS))
def test_driver_matches_the_restatement(golden_runs, mode, tmp_path):
    g = golden_runs["runs"][mode]
    inter, mins, _ = g["exp"]
    assert inter[0, 0] > 0 and inter[1, 1] > 0 and inter[0, 1] == inter[1, 0]
    r = kmx("dist", "--run", g["run"])      # shared is the default metric, standard output the default place
    assert r.returncode == 0, r.stderr
    assert r.stdout == dr.format_table(["D1", "D2"], "shared", inter)
    r = kmx("dist", "--run", g["run"], "--metric", "jaccard", "--output", tmp_path / "j.txt")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert open(tmp_path / "j.txt").read() == dr.format_table(["D1", "D2"], "jaccard", inter)
    if mins is not None:
        r = kmx("dist", "--run", g["run"], "--metric", "braycurtis")
        assert r.returncode == 0, r.stderr
        assert r.stdout == dr.format_table(["D1", "D2"], "braycurtis", inter, mins)
    else:
        r = kmx("dist", "--run", g["run"], "--metric", "braycurtis")
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("mode", ["kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin"])
def test_driver_lz4(golden_runs, mode, tmp_path):
    """a run written with --cpr gives the same text"""
    r = kmx(*golden_runs["base"], "--run-dir", tmp_path / "lz", "--mode", mode, "--cpr", *bloom(mode))
    assert r.returncode == 0, r.stderr
    ext = dr.KINDS[mode][0]
    name = tmp_path / "lz" / "matrices" / (f"matrix_0.{ext}.lz4" if mode.startswith("kmer") else f"matrix_0.{ext}")
    assert open(name, "rb").read()[12] == 1      # the header says: an lz4 body
    inter, mins, _ = golden_runs["runs"][mode]["exp"]
    for metric in ("shared", "jaccard") + (("braycurtis",) if mins is not None else ()):
        r = kmx("dist", "--run", tmp_path / "lz", "--metric", metric)
        assert r.returncode == 0 and r.stdout == dr.format_table(["D1", "D2"], metric, inter, mins), r.stderr


def test_driver_row_runs_and_shards(golden_runs):
    """a count run whose matrices need several runs of rows at --batch-mb 1 (4 000 random reads as one sample, golden sample 1 as the
    other, as test_kquery_gpu.py's big_run makes one); two shards on one device (--gpus 2): the same text"""
    import orc
    import kquery_ref as kr
    d = golden_runs["dir"]
    rep = orc.repart_static(10, 4)
    with open(d / "static.minimRepart", "wb") as f:
        f.write(struct.pack("<HQH", 4, len(rep), 1)); f.write(rep.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    reads = kr.random_reads(41, 4000, 150)
    with open(d / "big.fasta", "w") as f:
        f.write("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    with open(d / "big.fof", "w") as f:
        f.write(f"S1 : {d}/big.fasta\nS2 : {GD}/1.fasta\n")
    base = [{"in.fof": d / "big.fof", "fixture.minimRepart": d / "static.minimRepart"}.get(os.path.basename(str(a)), a) for a in golden_runs["base"]]
    r = kmx(*base, "--run-dir", d / "big", "--mode", "kmer:count:bin")
    assert r.returncode == 0, r.stderr
    inter, mins, total = expected_of(d / "big", "kmer:count:bin")
    assert total > (2 << 20)
    for metric in ("shared", "braycurtis"):
        want = dr.format_table(["S1", "S2"], metric, inter, mins)
        r = kmx("dist", "--run", d / "big", "--metric", metric)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        r = kmx("dist", "--run", d / "big", "--metric", metric, "--batch-mb", 1, "-v")
        assert r.returncode == 0 and r.stdout == want, r.stderr
        mt = re.search(r"runs of (\d+) rows", r.stderr)
        assert mt and int(mt.group(1)) * 16 * 4 < total, r.stderr      # 16-byte rows, four partitions: more than one run a partition
        r = kmx("dist", "--run", d / "big", "--metric", metric, "--gpus", 2, "--batch-mb", 1)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        r = kmx("dist", "--run", d / "big", "--metric", metric, "--gpus", 2)
        assert r.returncode == 0 and r.stdout == want, r.stderr


def test_driver_refusals(golden_runs, tmp_path):
    count, pa = golden_runs["runs"]["kmer:count:bin"]["run"], golden_runs["runs"]["kmer:pa:bin"]["run"]

    def refused(*args, word=None):
        r = kmx("dist", *args)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
        assert word is None or word in r.stderr, (args, r.stderr)

    refused()
    refused("--run", tmp_path, word="not a kmtricks runtime directory")
    r = kmx(*golden_runs["base"], "--run-dir", tmp_path / "bfc", "--mode", "hash:bfc:bin", "--bitw", 2, *bloom("hash:bfc:bin"))
    assert r.returncode == 0, r.stderr
    refused("--run", tmp_path / "bfc", word="hash:bfc:bin")
    refused("--run", pa, "--metric", "braycurtis", word="braycurtis")
    refused("--run", count, "--gpus", 0, word="--gpus")
    refused("--run", count, "--gpus", 17, word="--gpus")
    shutil.copytree(count, tmp_path / "cut")
    with open(tmp_path / "cut" / "matrices" / "matrix_2.count", "r+b") as f:
        f.truncate(os.path.getsize(tmp_path / "cut" / "matrices" / "matrix_2.count") - 3)
    refused("--run", tmp_path / "cut", word="matrix_2.count")
    shutil.copytree(pa, tmp_path / "cols")
    with open(tmp_path / "cols" / "matrices" / "matrix_0.pa", "r+b") as f:
        f.seek(29); f.write(struct.pack("<I", 3))
    refused("--run", tmp_path / "cols", word="matrix_0.pa")
