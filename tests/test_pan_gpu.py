"""`kmx pan` on the MI355X against tests/pan_ref.py: the C ABI through kmtricks_amd.lib on the bodies of pan_ref.gpu_cases() -- both tables
compared bit for bit --, accumulation into the caller's tables, the limits, the launch shapes the two knobs of pan.hip force, and the
driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr
import pan_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = pr.MODE_COUNT, pr.MODE_PA


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, what, shared=True):
    spec, sh = exp
    assert out.spectrum.dtype == np.uint64 and out.spectrum.tobytes() == spec.tobytes(), f"{what}: the spectrum\n{out.spectrum}\n{spec}"
    if shared:
        assert out.shared.shape == sh.shape and out.shared.tobytes() == sh.tobytes(), f"{what}: the shared table, first difference at {np.argwhere(out.shared != sh)[:3].tolist()}"
    else:
        assert out.shared is None


def algo_bytes(c, shared):
    M1, body = c.n_use + 1, c.n_rows * dr.row_bytes(c.key_words, c.n_cols, c.mode)
    return body + 24 * M1 + (body + 24 * c.n_rows + 8 * M1 * c.n_cols if shared else 0)


@pytest.mark.parametrize("name", [c.name for c in pr.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of a byte, of a wave's worth of units, of a column block of k_pan_shared and of the M that ends the LDS
    histograms; rows on both sides of a wave's chunk and of a run of the order; recurrence shapes with few, with every and with one class;
    lists in every order; key widths, so that rows fall at every alignment; PA padding bits all set; counts of 2^32 - 1 with min_abund
    1, 2, 2^32 - 1.  With and without KMX_PAN_SHARED: the spectrum does not depend on the flag"""
    c = pr.case(name)
    for a, exp in c.expected.items():
        out = ctx.pan(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a, shared=True)
        same(out, exp, f"{name} a={a}")
        assert out.algo_bytes == algo_bytes(c, True)
        pr.check_identities(out.spectrum, out.shared, c.n_rows, c.cols, c.n_cols)
        plain = ctx.pan(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a)
        same(plain, exp, f"{name} a={a} without the flag", shared=False)
        assert plain.algo_bytes == algo_bytes(c, False)


ODD = ["c-65-none-r12293-k2-skewed", "c-130-scattered-r257-k3-skewed", "p-9-one-r4200-k2-skewed", "p-520-one-r700-k3-skewed", "c-7-none-r255-k4-uniform",
       "p-65-reversed-r12293-k1-uniform-long"]


@pytest.mark.parametrize("name", ODD)
def test_body_at_an_odd_host_address_and_device_resident(ctx, name):
    """the body handed in at an odd host address, and through _dev from every device alignment: the same tables"""
    import torch
    c = pr.case(name)
    a = next(iter(c.expected))
    exp = c.expected[a]
    buf = np.zeros(len(c.body) + 9, np.uint8)
    for shift in (1, 3):
        view = buf[shift:shift + len(c.body)]
        view[:] = c.body
        assert view.ctypes.data % 2 == 1
        same(ctx.pan(view, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a, shared=True), exp, (name, "host", shift))
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 3):
        d = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        d[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        same(ctx.pan_dev(d.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a, shared=True), exp, (name, "dev", shift))


@pytest.mark.parametrize("mode,N,kind", [(COUNT, 65, "scattered"), (PA, 130, "reversed"), (COUNT, 300, "none"), (PA, 9, "none")])
def test_two_calls_into_the_callers_tables(ctx, mode, N, kind):
    """one call, against two calls over a cut into tables of the caller's that hold 2^32 - 1 in every cell: an add carries into the
    high word, unlisted columns and row 0 of shared stay as they were"""
    import torch
    rows, kw, cut = 1500, 2, 389
    body = pr.shaped_body(77 + N, rows, N, kw, mode, "uniform")
    cols = pr.make_cols(kind, N, 5)
    M = N if cols is None else len(cols)
    rb = dr.row_bytes(kw, N, mode)
    spec, sh = pr.pan_expected_np(body, N, kw, mode, cols)
    same(ctx.pan(body, rows, N, kw, mode, cols=cols, shared=True), (spec, sh), "one call")
    dev = torch.device("cuda:0")
    seed = 0xFFFFFFFF
    d_spec = torch.full((3, M + 1), seed, dtype=torch.int64, device=dev)
    d_sh = torch.full((M + 1, N), seed, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    first = ctx.pan(body[:cut * rb], cut, N, kw, mode, cols=cols, spectrum_dev=d_spec.data_ptr(), shared_dev=d_sh.data_ptr(), keep=True)
    try:
        assert first.spectrum_dev() == d_spec.data_ptr() and first.shared_dev() == d_sh.data_ptr()
        second = ctx.pan(body[cut * rb:], rows - cut, N, kw, mode, cols=cols, spectrum_dev=d_spec.data_ptr(), shared_dev=d_sh.data_ptr())
    finally:
        first.free()
    torch.cuda.synchronize()
    got_spec, got_sh = d_spec.cpu().numpy().view(np.uint64), d_sh.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_spec, spec + np.uint64(seed)) and np.array_equal(got_sh, sh + np.uint64(seed))
    assert np.array_equal(second.spectrum, got_spec) and np.array_equal(second.shared, got_sh)      # the table as it stands
    assert (got_spec >> np.uint64(32)).any() and (got_sh >> np.uint64(32)).any()      # adds carried
    assert (got_sh[0] == seed).all()
    # the spectrum alone into the caller's table, no shared table
    d_spec.fill_(seed)
    torch.cuda.synchronize()
    out = ctx.pan(body, rows, N, kw, mode, cols=cols, spectrum_dev=d_spec.data_ptr())
    assert out.shared is None and np.array_equal(out.spectrum, spec + np.uint64(seed))


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, a=1, flags=0, n_rows=0, shared=None):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        M = (N if cc is None else len(cc)) if M is None else M
        for fn in (lib._lib.kmx_pan_host, lib._lib.kmx_pan_dev):
            t = lib.KmxPanTask(kw, mode, N, M, None, n_rows, None if cc is None else cc.ctypes.data, a, flags, None, shared)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, a, flags, n_rows, shared)

    OK, INVAL, UNSUP = 0, -2, -5
    call(INVAL, N=0, cols=None); call(INVAL, M=0)
    call(INVAL, N=2, cols=(0, 1, 0))                               # n_use > n_cols
    call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4))       # an index at N; a duplicate
    call(INVAL, cols=None, M=8)                                    # the identity with M != N
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, mode=7)
    call(INVAL, a=0); call(INVAL, a=0, mode=PA); call(INVAL, a=2, mode=PA)
    call(INVAL, flags=2); call(INVAL, flags=0x80000001)
    call(INVAL, shared=0x1000)                                     # a shared table without the flag
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode); call(UNSUP, mode=mode, kw=0)
    call(UNSUP, N=2 ** 30, cols=None)                              # a row of 8 + 2^32 bytes
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32 - 255, mode=PA)
    call(UNSUP, N=2 ** 15, cols=None, flags=lib.PAN_SHARED)        # (2^15 + 1) * 2^15 * 8 bytes: 8 GiB and more
    call(UNSUP, N=2 ** 15, cols=None, flags=lib.PAN_SHARED, mode=PA)
    # what is valid is taken: no rows; the largest shared table below the limit is not asked for here (it would be allocated)
    for flags in (0, lib.PAN_SHARED):
        t = lib.KmxPanTask(1, COUNT, 9, 3, None, 0, np.array([4, 2, 1], np.uint32).ctypes.data, 1, flags, None, None)
        res = C.c_void_p()
        assert lib._lib.kmx_pan_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
        spec = np.ones((3, 4), np.uint64)
        assert lib._lib.kmx_pan_result_copy_spectrum(res, spec.ctypes.data, spec.size) == OK and not spec.any()      # n_rows = 0 adds nothing
        sh = np.ones((4, 9), np.uint64)
        assert lib._lib.kmx_pan_result_copy_shared(res, sh.ctypes.data, sh.size) == (OK if flags else INVAL) and sh.any() != bool(flags)
        assert lib._lib.kmx_pan_result_copy_spectrum(res, spec.ctypes.data, spec.size - 1) == INVAL
        lib._lib.kmx_pan_result_free(res)
    # the context stays usable
    c = pr.case(next(x.name for x in pr.gpu_cases() if x.name.startswith("c-9-")))
    a = next(iter(c.expected))
    same(ctx.pan(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a, shared=True), c.expected[a], c.name)


# ---- the launch shapes KMX_PAN_CUS and KMX_PAN_GRID force ------------------------------------------------------------------------
def launch_shape(n_rows, N, mode, cus, grid_cap):
    """the launcher's formulas (pan.hip, pan_queue) -> trips of each stride loop, and the runs a column block of k_pan_shared takes"""
    units = N if mode == COUNT else (N + 7) // 8
    L = 1
    while L < 64 and L < units:
        L <<= 1
    RW = 64
    if L == 64:
        while RW > 4 and n_rows // RW < cus * 4 * 8:
            RW >>= 1
    chunks = (n_rows + RW - 1) // RW
    score_grid = min((chunks + 3) // 4, min(min(cus * 8, 1 << 16), grid_cap))
    tiles = (n_rows + 255) // 256
    order_grid = min(tiles, grid_cap)
    n_blocks = (units + 255) // 256
    runs = (n_rows + 255) // 256
    shared_grid = min(runs * n_blocks, grid_cap)
    return dict(score=-(-chunks // (4 * score_grid)), order=-(-tiles // order_grid), shared=-(-(runs * n_blocks) // shared_grid), runs=runs, blocks=n_blocks)


@pytest.mark.parametrize("mode,N,rows,kind", [(COUNT, 300, 2100, "scattered"), (PA, 2100, 2100, "none"), (COUNT, 40, 4200, "reversed"), (PA, 64, 4200, "scattered")])
def test_launch_shapes(ctx, mode, N, rows, kind, monkeypatch):
    """KMX_PAN_CUS=1 and KMX_PAN_GRID=3 (read per call): several trips of each stride loop and several runs a column block; each shape
    against the reference and, byte for byte, against the same call with the knobs unset"""
    kw = 1
    body = pr.shaped_body(1234 + N, rows, N, kw, mode, "uniform")
    cols = pr.make_cols(kind, N, 9)
    exp = pr.pan_expected_np(body, N, kw, mode, cols)
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.delenv("KMX_PAN_CUS", raising=False); monkeypatch.delenv("KMX_PAN_GRID", raising=False)
    base = ctx.pan(body, rows, N, kw, mode, cols=cols, shared=True)
    same(base, exp, "knobs unset")
    for env in (dict(KMX_PAN_CUS="1"), dict(KMX_PAN_GRID="3"), dict(KMX_PAN_CUS="1", KMX_PAN_GRID="3")):
        shape = launch_shape(rows, N, mode, 1 if "KMX_PAN_CUS" in env else n_cu, 3 if "KMX_PAN_GRID" in env else 1 << 16)
        assert shape["score"] > 1 and shape["runs"] > 1, (env, shape)
        if "KMX_PAN_GRID" in env:
            assert shape["order"] > 1 and shape["shared"] > 1, (env, shape)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.pan(body, rows, N, kw, mode, cols=cols, shared=True)
        for k in env:
            monkeypatch.delenv(k)
        same(out, exp, env)
        assert out.spectrum.tobytes() == base.spectrum.tobytes() and out.shared.tobytes() == base.shared.tobytes()


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
    d = tmp_path_factory.mktemp("kmxpan")
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


def restated(run, mode, cols, a=1):
    """the restatement on the run's bodies, summed over the partitions -> (spectrum, shared, rows)"""
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, 4, 31)
    parts = [pr.pan_expected_np(b, n, kw, rmode, cols, a) for b in bodies]
    rows = sum(len(b) for b in bodies) // dr.row_bytes(kw, n, rmode)
    return sum(p[0] for p in parts), sum(p[1] for p in parts), rows


def check_driver(r, tmp_path, ids, cols, a, spec, shared, rows):
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "spec.tsv").read() == pr.spectrum_text(ids, a, spec)
    assert open(tmp_path / "shared.tsv").read() == pr.shared_text(ids, cols, shared)
    head, lines = pr.parse_curves(r.stdout)
    assert head["samples"] == str(len(ids)) and head["rows"] == str(rows) and head["min_abund"] == str(a) and int(spec[0].sum()) == rows
    exact = pr.curves_exact(spec)
    for m, sid, pan, core, new, pan_o, core_o in lines:
        assert sid == ids[m - 1] and pan_o == exact["pan_order"][m] and core_o == exact["core_order"][m]
        for got, key in ((pan, "pan_mean"), (core, "core_mean"), (new, "new_mean")):
            assert abs(float(got) - float(exact[key][m])) <= 1e-9 * rows + 5e-7, (m, key)
    # the spectrum file read back gives the same curves
    again = kmx("pan", "--from-spectrum", tmp_path / "spec.tsv")
    assert again.returncode == 0 and again.stdout == r.stdout


@pytest.mark.parametrize("mode", KINDS)
def test_driver_on_the_golden_samples(golden_runs, mode, tmp_path):
    """with and without --samples, --min-abund 2, --shared, --spectrum and --gpus 2, against pan_ref applied to the run's matrices; the
    spectrum file read back with --from-spectrum prints the same curves"""
    run = golden_runs["runs"][mode]
    outs = ("--spectrum", tmp_path / "spec.tsv", "--shared", tmp_path / "shared.tsv")
    spec, shared, rows = restated(run, mode, None)
    assert rows > 100 and spec[0][1] > 0 and spec[0][2:].sum() > 0 and spec[0][0] == 0      # private and shared rows; every row is some sample's
    r = kmx("pan", "--run", run, *outs, "-v")
    check_driver(r, tmp_path, IDS, None, 1, spec, shared, rows)
    assert "3 of 3 samples, 4 partitions" in r.stderr
    one = r.stdout
    r = kmx("pan", "--run", run, *outs, "--gpus", 2)
    check_driver(r, tmp_path, IDS, None, 1, spec, shared, rows)
    assert r.stdout == one
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D3\n\nD1\n")
    spec, shared, rows2 = restated(run, mode, [2, 0])
    r = kmx("pan", "--run", run, *outs, "--samples", tmp_path / "s.txt", "--output", tmp_path / "curves.tsv")
    assert r.stdout == "" and rows2 == rows
    r.stdout = open(tmp_path / "curves.tsv").read()
    check_driver(r, tmp_path, ["D3", "D1"], [2, 0], 1, spec, shared, rows)
    if mode == "kmer:count:bin":
        spec2, shared2, _ = restated(run, mode, [2, 0], a=2)
        assert not np.array_equal(spec2, spec)
        r = kmx("pan", "--run", run, *outs, "--samples", tmp_path / "s.txt", "--min-abund", 2)
        check_driver(r, tmp_path, ["D3", "D1"], [2, 0], 2, spec2, shared2, rows)


def test_driver_row_runs_and_lz4(golden_runs, tmp_path):
    """a --cpr run gives what the plain run gives; --batch-mb 1 cuts every partition of a hand-made run (100 count columns, 3000 rows a
    partition) into runs of 1248 rows, on one shard and on two"""
    run = golden_runs["runs"]["kmer:count:bin"]
    r = kmx(*golden_runs["base"], "--file", golden_runs["dir"] / "in.fof", "--run-dir", tmp_path / "lz", "--mode", "kmer:count:bin", "--cpr")
    assert r.returncode == 0, r.stderr
    outs = ("--spectrum", tmp_path / "spec.tsv", "--shared", tmp_path / "shared.tsv")
    spec, shared, rows = restated(run, "kmer:count:bin", None)
    check_driver(kmx("pan", "--run", tmp_path / "lz", *outs), tmp_path, IDS, None, 1, spec, shared, rows)
    # 1 MB: two runs in flight, 512 KB each -- rows of 8 + 4 * 100 bytes + 12: 1248 rows a run, 3000 rows a partition
    ids = [f"S{j}" for j in range(100)]
    bodies = [pr.shaped_body(40 + p, 3000, 100, 1, COUNT, "uniform") for p in range(3)]
    root = dr.write_run(tmp_path / "wide", "hash:count:bin", 31, ids, bodies, window=16)
    parts = [pr.pan_expected_np(b, 100, 1, COUNT) for b in bodies]
    spec, shared = sum(p[0] for p in parts), sum(p[1] for p in parts)
    r = kmx("pan", "--run", root, *outs, "--batch-mb", 1, "-v")
    check_driver(r, tmp_path, ids, None, 1, spec, shared, 9000)
    assert "runs of 1248 rows" in r.stderr
    r2 = kmx("pan", "--run", root, *outs, "--batch-mb", 1, "--gpus", 2)
    assert r2.returncode == 0 and r2.stdout == r.stdout
