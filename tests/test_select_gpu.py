"""`kmx select` on the MI355X against tests/select_ref.py: the C ABI through kmtricks_amd.lib on the bodies of select_ref.gpu_cases() -- the
kept body and every record compared exactly --, the two movers against each other, the limits, composition on device-resident bodies,
and the driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr
import select_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = sr.MODE_COUNT, sr.MODE_PA


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, c, what):
    body, recs = exp
    assert out.recs["row"].tolist() == recs["row"].tolist(), f"{what}: kept rows ({len(out.recs)}, expected {len(recs)})"
    assert out.recs["rec"].tolist() == recs["rec"].tolist(), f"{what}: recurrences"
    assert out.body == body, f"{what}: the kept body"
    orb = len(body) // len(recs) if len(recs) else 0
    assert out.algo_bytes == c.n_rows * dr.row_bytes(c.key_words, c.n_cols, c.mode) + len(recs) * (orb + 8), what


@pytest.mark.parametrize("name", [c.name for c in sr.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of a byte and of a wave's worth of units, lists in every order; rows on both sides of a wave's chunk and of a
    placement tile; key widths, so that PA rows and output rows fall at every alignment; input padding bits all set; fills 0 ... 1 and
    counts of 2^32 - 1; min_abund 1, 2, 2^32 - 1; the five recurrence ranges; ZERO_BELOW on and off"""
    c = sr.case(name)
    for r, exp in zip(c.runs, c.expected):
        out = ctx.select(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, **r)
        same(out, exp, c, f"{name} {r}")
        assert len(out.body) == len(out.recs) * sr.out_row_bytes(c.key_words, c.n_out, c.out_mode)


@pytest.mark.parametrize("name", ["cc-65-perm-63", "cp-130-perm-64", "pp-9-perm-8", "pp-520-every-other-260", "cc-subset", "pp-subset"])
def test_body_at_an_odd_host_address_and_device_resident(ctx, name):
    """the body handed in at an odd host address, and through _dev from every device alignment: the same bytes"""
    import torch
    c = next(x for x in sr.gpu_cases() if x.name.startswith(name))
    r = c.runs[1] if len(c.runs) > 2 else c.runs[0]
    exp = sr.select_expected_np(c.body, c.n_cols, c.key_words, c.mode, c.cols, **r)
    buf = np.zeros(len(c.body) + 9, np.uint8)
    for shift in (1, 3):
        view = buf[shift:shift + len(c.body)]
        view[:] = c.body
        assert view.ctypes.data % 2 == 1
        same(ctx.select(view, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, **r), exp, c, (name, "host", shift))
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 3):
        d = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        d[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        same(ctx.select_dev(d.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, **r), exp, c, (name, "dev", shift))


@pytest.mark.parametrize("mode,N,kw", [(COUNT, 9, 1), (COUNT, 130, 3), (PA, 64, 2), (PA, 520, 1)])
def test_both_movers_agree(ctx, mode, N, kw):
    """the list left out takes k_filter_move (rows moved whole); the identity said aloud takes k_select_move: the same bytes, at 0.1 %,
    about half and all of the rows kept, over several placement tiles"""
    body = sr.make_body(31 + N, 2100, N, kw, mode, fill=0.5, maxed=0.05, lo=1, hi=4)
    recs = sr.select_expected_np(body, N, kw, mode)[1]["rec"]
    med, top = int(np.median(recs)), int(np.sort(recs)[-3])
    for lo, hi in ((0, None), (med, None), (top, None), (0, med), (2, 1)):
        kw_args = dict(min_rec=lo, max_rec=hi)
        whole = ctx.select(body, 2100, N, kw, mode, cols=None, **kw_args)
        said = ctx.select(body, 2100, N, kw, mode, cols=np.arange(N), **kw_args)
        exp = sr.select_expected_np(body, N, kw, mode, None, **kw_args)
        assert whole.body == said.body == exp[0] and whole.recs.tobytes() == said.recs.tobytes() == exp[1].tobytes(), (mode, N, lo, hi)
        if mode == COUNT:      # ZERO_BELOW with a = 1 changes no count and takes the general road too
            zb = ctx.select(body, 2100, N, kw, mode, cols=None, zero_below=True, **kw_args)
            assert zb.body == exp[0] and zb.recs.tobytes() == exp[1].tobytes()
    assert 0 < (recs >= top).sum() < 30 and 0.3 < (recs >= med).mean() < 0.8


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    c = next(x for x in sr.gpu_cases() if x.name.startswith("cc-9-perm-8"))

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, a=1, out_mode=None, flags=0, n_rows=0):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        M = (N if cc is None else len(cc)) if M is None else M
        for fn in (lib._lib.kmx_select_host, lib._lib.kmx_select_dev):
            t = lib.KmxSelectTask(kw, mode, N, M, None, n_rows, None if cc is None else cc.ctypes.data, a, 0, 0xFFFFFFFF,
                                  mode if out_mode is None else out_mode, flags, 0)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, a, out_mode, flags, n_rows)

    OK, INVAL, UNSUP = 0, -2, -5
    call(INVAL, N=0, cols=None); call(INVAL, M=0)
    call(INVAL, N=2, cols=(0, 1, 0))                               # n_out > n_cols
    call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4))       # an index at N; a duplicate
    call(INVAL, cols=None, M=8)                                    # the identity with M != N
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, mode=7); call(INVAL, out_mode=7); call(INVAL, out_mode=lib.MODE_BF)
    call(INVAL, mode=PA, out_mode=COUNT)
    call(INVAL, a=0); call(INVAL, a=0, mode=PA); call(INVAL, a=2, mode=PA)
    call(INVAL, flags=lib.SELECT_ZERO_BELOW, out_mode=PA); call(INVAL, flags=lib.SELECT_ZERO_BELOW, mode=PA)
    call(INVAL, flags=2); call(INVAL, flags=0x80000001)
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode)
    call(UNSUP, N=2 ** 30, cols=None)                              # a row of 8 + 2^32 bytes
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32, mode=PA)
    # what is valid is taken: no rows, min_rec above max_rec
    t = lib.KmxSelectTask(1, COUNT, 9, 9, None, 0, None, 1, 2, 1, COUNT, 0, 0)
    res = C.c_void_p()
    assert lib._lib.kmx_select_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
    assert lib._lib.kmx_select_result_rows(res) == 0 and lib._lib.kmx_select_result_row_bytes(res) == 44
    lib._lib.kmx_select_result_free(res)
    # the context stays usable
    same(ctx.select(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, **c.runs[0]), c.expected[0], c, c.name)


@pytest.mark.parametrize("mode,out_mode", sr.MODE_PAIRS)
def test_composition_on_device_resident_bodies(ctx, mode, out_mode):
    """select_dev on the body_dev of a previous select: select(cols B) o select(cols A) equals select(A[B]) when no row filter is set"""
    N, kw, rows = 70, 2, 600
    body = sr.make_body(5, rows, N, kw, mode, fill=0.4, maxed=0.05, lo=1, hi=4)
    rng = np.random.default_rng(3)
    A = rng.permutation(N)[:33].astype(np.uint32)
    B = rng.permutation(33)[:12].astype(np.uint32)
    first = ctx.select(body, rows, N, kw, mode, cols=A, out_mode=mode, keep=True)      # the counts stay counts for the second step
    try:
        assert first.rows() == rows and first.row_bytes() == dr.row_bytes(kw, 33, mode)
        second = ctx.select_dev(first.body_dev(), rows, 33, kw, mode, cols=B, out_mode=out_mode)
    finally:
        first.free()
    direct = ctx.select(body, rows, N, kw, mode, cols=A[B], out_mode=out_mode)
    exp = sr.select_expected_np(body, N, kw, mode, A[B], out_mode=out_mode)
    assert second.body == direct.body == exp[0] and second.recs.tobytes() == direct.recs.tobytes() == exp[1].tobytes()


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


KINDS = ("kmer:count:bin", "kmer:pa:bin")
IDS = ["D1", "D2", "D3"]


def matrix_files(run, mode, n_parts=4):
    ext = dr.KINDS[mode][0]
    return [open(os.path.join(str(run), "matrices", f"matrix_{p}.{ext}"), "rb").read() for p in range(n_parts)]


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples and a third made of slices of both, 4 partitions, with the fixture's
    repartition table: every k-mer of every sample is a row (the merge's soft-min 1, recurrence-min 1, no rescue)"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxselect")
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


def restated(run, mode, cols, out_mode=None, **args):
    """the restatement on the source's bodies -> the bodies `kmx select` must write"""
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, 4, 31)
    return [sr.select_expected_np(b, n, kw, rmode, cols, out_mode=out_mode, **args)[0] for b in bodies], kw


@pytest.mark.parametrize("mode", KINDS)
def test_driver_all_samples_is_the_source(golden_runs, mode, tmp_path):
    """all samples, a = 1, --min-rec 0: every matrix file is the source's, byte for byte; and the directory is a run directory"""
    run = golden_runs["runs"][mode]
    r = kmx("select", "--run", run, "--output", tmp_path / "all", "--min-rec", 0, "-v")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert matrix_files(tmp_path / "all", mode) == matrix_files(run, mode)
    rows = sum(len(b) for b in dr.read_run_bodies(run, mode, 4, 31)[0]) // dr.row_bytes(1, 3, dr.KINDS[mode][5])
    assert f"total: {rows} rows in, {rows} kept" in r.stderr and "partition 3:" in r.stderr
    for name in ("kmtricks.fof", "options.txt", "repartition_gatb/repartition.minimRepart", "hash.info", "config_gatb/gatb.config"):
        assert open(tmp_path / "all" / name, "rb").read() == open(run / name, "rb").read(), name


@pytest.mark.parametrize("mode", KINDS)
@pytest.mark.parametrize("subset", [("D3", "D1"), ("D2",)])
def test_driver_subset_is_the_pipeline_on_the_subset(golden_runs, mode, subset, tmp_path):
    """--samples S with --min-rec 1: the matrices of `kmx pipeline` run on S alone, in S's order, with the same table"""
    d, run = golden_runs["dir"], golden_runs["runs"][mode]
    lines = {ln.split()[0]: ln for ln in open(d / "in.fof").read().splitlines()}
    with open(tmp_path / "s.txt", "w") as f:
        f.write("".join(s + "\n" for s in subset))
    with open(tmp_path / "s.fof", "w") as f:
        f.write("".join(lines[s] + "\n" for s in subset))
    r = kmx(*golden_runs["base"], "--file", tmp_path / "s.fof", "--run-dir", tmp_path / "alone", "--mode", mode)
    assert r.returncode == 0, r.stderr
    r = kmx("select", "--run", run, "--output", tmp_path / "sel", "--samples", tmp_path / "s.txt", "--min-rec", 1)
    assert r.returncode == 0, r.stderr
    got, want = matrix_files(tmp_path / "sel", mode), matrix_files(tmp_path / "alone", mode)
    assert got == want and sum(len(x) for x in got) > 4 * 45
    assert open(tmp_path / "sel" / "kmtricks.fof").read() == open(tmp_path / "s.fof").read()
    cols = [IDS.index(s) for s in subset]
    exp, kw = restated(run, mode, cols, min_rec=1)
    assert [x[45:] for x in got] == exp
    assert sum(len(x) for x in exp) < sum(len(x) - 45 for x in matrix_files(run, mode))      # rows were dropped


def test_driver_pa_of_the_count_run_is_the_pa_run(golden_runs, tmp_path):
    """--pa on the count run equals the same selection on the PA run; fractions are of M; --zero-below and --min-abund as restated"""
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D2\nD3\nD1\n")
    cnt, pa = golden_runs["runs"]["kmer:count:bin"], golden_runs["runs"]["kmer:pa:bin"]
    args = ("--samples", tmp_path / "s.txt", "--min-frac", 0.5, "--max-frac", 0.7)      # ceil(1.5) = 2 ... floor(2.1) = 2
    r1 = kmx("select", "--run", cnt, "--output", tmp_path / "a", "--pa", *args)
    r2 = kmx("select", "--run", pa, "--output", tmp_path / "b", *args)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    got = matrix_files(tmp_path / "a", "kmer:pa:bin")
    assert got == matrix_files(tmp_path / "b", "kmer:pa:bin")
    exp, _ = restated(pa, "kmer:pa:bin", [1, 2, 0], min_rec=2, max_rec=2)
    assert [x[45:] for x in got] == exp and 0 < sum(len(x) for x in exp) < sum(len(x) - 45 for x in matrix_files(pa, "kmer:pa:bin"))
    assert ", mode=pa," in open(tmp_path / "a" / "options.txt").read() and ", mode=count," in open(cnt / "options.txt").read()
    assert open(tmp_path / "a" / "options.txt").read() == open(cnt / "options.txt").read().replace(", mode=count,", ", mode=pa,")
    for zb in (False, True):
        out = tmp_path / f"z{int(zb)}"
        r = kmx("select", "--run", cnt, "--output", out, "--samples", tmp_path / "s.txt", "--min-abund", 2, "--min-rec", 1, *(("--zero-below",) if zb else ()))
        assert r.returncode == 0, r.stderr
        exp, _ = restated(cnt, "kmer:count:bin", [1, 2, 0], min_abund=2, min_rec=1, zero_below=zb)
        assert [x[45:] for x in matrix_files(out, "kmer:count:bin")] == exp and sum(len(x) for x in exp) > 0


@pytest.mark.parametrize("mode", KINDS)
def test_downstream_commands_read_the_output(golden_runs, mode, tmp_path):
    """`kmx dist --metric shared` on a column-only selection is the sub-table of `kmx dist` on the source; `kmx dump` and `kmx aggregate`
    print the restatement's rows"""
    run = golden_runs["runs"][mode]
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D3\nD1\n")
    r = kmx("select", "--run", run, "--output", tmp_path / "sel", "--samples", tmp_path / "s.txt")
    assert r.returncode == 0, r.stderr
    whole, part = kmx("dist", "--run", run), kmx("dist", "--run", tmp_path / "sel")
    assert whole.returncode == 0 and part.returncode == 0, (whole.stderr, part.stderr)
    table = [ln.split("\t") for ln in whole.stdout.splitlines()]
    assert table[0] == ["", "D1", "D2", "D3"]
    want = "\tD3\tD1\n" + "".join("\t".join([IDS[i]] + [table[1 + i][1 + j] for j in (2, 0)]) + "\n" for i in (2, 0))
    assert part.stdout == want
    # the rows as text: the key as the source's dump prints it, then the restated columns
    exp, kw = restated(run, mode, [2, 0])
    rmode, ext = dr.KINDS[mode][5], dr.KINDS[mode][0]
    lines = []
    for p, body in enumerate(exp):
        src = kmx("dump", "--input", run / "matrices" / f"matrix_{p}.{ext}")
        assert src.returncode == 0, src.stderr
        pay = dr.split_payload(body, 2, kw, rmode)
        mine = [ln.split(" ")[0] + "".join(f" {int(v)}" for v in row) + "\n" for ln, row in zip(src.stdout.splitlines(), pay)]
        assert len(mine) == len(src.stdout.splitlines()) == len(pay)      # (no row filter: the rows are the source's)
        got = kmx("dump", "--input", tmp_path / "sel" / "matrices" / f"matrix_{p}.{ext}")
        assert got.returncode == 0 and got.stdout == "".join(mine), got.stderr
        lines += mine
    agg = kmx("aggregate", "--run-dir", tmp_path / "sel", "--pa-matrix" if rmode == PA else "--matrix", "kmer")
    assert agg.returncode == 0 and agg.stdout == "".join(lines) and len(lines) > 100, agg.stderr


@pytest.mark.parametrize("mode", KINDS)
def test_driver_shards_row_runs_and_lz4(golden_runs, mode, tmp_path):
    """--gpus 2 equals --gpus 1, a --cpr source equals the plain one, and --cpr writes what unpacks to
    the plain output"""
    run = golden_runs["runs"][mode]
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D2\nD1\n")
    args = ("--samples", tmp_path / "s.txt", "--min-rec", 1, "--max-rec", 1)
    outs = {}
    r = kmx(*golden_runs["base"], "--file", golden_runs["dir"] / "in.fof", "--run-dir", tmp_path / "lz", "--mode", mode, "--cpr")
    assert r.returncode == 0, r.stderr
    for name, src, extra in (("one", run, ()), ("two", run, ("--gpus", 2)), ("lz", tmp_path / "lz", ()), ("cpr", run, ("--cpr",))):
        r = kmx("select", "--run", src, "--output", tmp_path / f"out_{name}", *args, *extra)
        assert r.returncode == 0, (name, r.stderr)
        if name != "cpr":
            outs[name] = matrix_files(tmp_path / f"out_{name}", mode)
    exp, _ = restated(run, mode, [1, 0], min_rec=1, max_rec=1)
    assert [x[45:] for x in outs["one"]] == exp and sum(len(x) for x in exp) > 0
    assert outs["two"] == outs["one"] and outs["lz"] == outs["one"]
    ext = dr.KINDS[mode][0]
    packed = open(tmp_path / "out_cpr" / "matrices" / f"matrix_0.{ext}.lz4", "rb").read()
    assert packed[12] == 1 and packed[:12] == outs["one"][0][:12] and packed[13:45] == outs["one"][0][13:45]
    again = kmx("select", "--run", tmp_path / "out_cpr", "--output", tmp_path / "again")      # read back through the driver: every sample, every row
    assert again.returncode == 0 and matrix_files(tmp_path / "again", mode) == outs["one"], again.stderr


def test_diff_query_and_combine_read_the_output(golden_runs, tmp_path):
    """`kmx combine` of two column selections is the selection of their columns side by side; `kmx diff` and `kmx query --kmer-index`
    take a selection as they take the source"""
    run = golden_runs["runs"]["kmer:count:bin"]
    for name, ids in (("a", ["D1"]), ("b", ["D3", "D2"]), ("c", ["D1", "D3", "D2"])):
        with open(tmp_path / f"{name}.txt", "w") as f:
            f.write("".join(s + "\n" for s in ids))
        r = kmx("select", "--run", run, "--output", tmp_path / name, "--samples", tmp_path / f"{name}.txt")
        assert r.returncode == 0, r.stderr
    with open(tmp_path / "runs.fof", "w") as f:
        f.write(f"{tmp_path / 'a'}\n{tmp_path / 'b'}\n")
    r = kmx("combine", "--fof", tmp_path / "runs.fof", "--output", tmp_path / "joined")
    assert r.returncode == 0, r.stderr
    assert matrix_files(tmp_path / "joined", "kmer:count:bin") == matrix_files(tmp_path / "c", "kmer:count:bin")
    with open(tmp_path / "groups.txt", "w") as f:
        f.write("D3 control\nD1 case\n")
    whole = kmx("diff", "--run", run, "--groups", tmp_path / "groups.txt", "--correction", "none", "--alpha", 0.9)
    part = kmx("diff", "--run", tmp_path / "c", "--groups", tmp_path / "groups.txt", "--correction", "none", "--alpha", 0.9)
    assert whole.returncode == 0 and part.returncode == 0 and part.stdout == whole.stdout and len(part.stdout.splitlines()) > 1, (whole.stderr, part.stderr)
    q = kmx("query", "--kmer-index", tmp_path / "b", "--query", os.path.join(GD, "2.fasta"), "--format", "sums")
    assert q.returncode == 0 and len(q.stdout.splitlines()) >= 2, q.stderr
