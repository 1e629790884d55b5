"""`kmx spectra` on the MI355X against tests/spectra_ref.py: the C ABI through kmtricks_amd.lib on the bodies of spectra_ref.gpu_cases() --
both tables compared bit for bit, with either flag alone and with both --, accumulation into the caller's tables, the limits, the launch
shapes the two knobs of spectra.hip force, and the driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr
import spectra_ref as sr

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


def same(out, exp, what, hist=True, joint=True):
    eh, ej = exp
    if hist:
        assert out.hist.dtype == np.uint64 and out.hist.shape == eh.shape and out.hist.tobytes() == eh.tobytes(), f"{what}: hist, first difference at {np.argwhere(out.hist != eh)[:3].tolist()}"
    else:
        assert out.hist is None
    if joint:
        assert out.joint.dtype == np.uint64 and out.joint.shape == ej.shape and out.joint.tobytes() == ej.tobytes(), f"{what}: joint, first difference at {np.argwhere(out.joint != ej)[:3].tolist()}"
    else:
        assert out.joint is None


def call(ctx, c, body=None, hist=True, joint=True, **kw):
    return ctx.spectra(c.body if body is None else body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, cap=c.cap, pairs=c.pairs if joint else None,
                       joint_cap=c.joint_cap, hist=hist, **kw)


@pytest.mark.parametrize("name", [c.name for c in sr.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of a byte, of a wave and of a column block; rows on both sides of a wave and of a tile; key widths, so that
    rows fall at every alignment; PA padding bits all set; bodies of zeros, of equal rows, of few and of every value alike, with counts of
    C - 1, C, C + 1 and 2^32 - 1; both caps on either side of what LDS holds; pair counts around a group; both roads of JOINT.  Both
    flags, and each alone: the tables do not depend on the other flag"""
    c = sr.case(name)
    out = call(ctx, c)
    same(out, c.expected, name)
    assert out.algo_bytes == c.algo_bytes()
    h = call(ctx, c, joint=False)
    same(h, c.expected, name + " HIST alone", joint=False)
    assert h.algo_bytes == c.algo_bytes(joint=False)
    j = call(ctx, c, hist=False)
    same(j, c.expected, name + " JOINT alone", hist=False)
    assert j.algo_bytes == c.algo_bytes(hist=False)


def pick(pred):
    return next(c.name for c in sr.gpu_cases() if pred(c))


ODD = [pick(lambda c: c.mode == COUNT and c.n_rows == 4200 and c.plan["stream"] and c.cap <= sr.HIST_LDS_CAP and c.shape == "uniform"),
       pick(lambda c: c.mode == COUNT and c.n_rows >= 700 and not c.plan["stream"] and c.cap <= sr.HIST_LDS_CAP),
       pick(lambda c: c.mode == COUNT and c.n_rows == 4200 and c.cap > sr.HIST_LDS_CAP and c.shape != "zero"),
       pick(lambda c: c.mode == PA and c.n_rows == 4200 and c.plan["stream"] and c.shape == "uniform"),
       pick(lambda c: c.mode == PA and c.n_rows >= 700 and not c.plan["stream"]),
       pick(lambda c: c.mode == COUNT and 0 < c.n_rows <= 257 and c.key_words == 3 and c.n_cols > 8)]


@pytest.mark.parametrize("name", ODD)
def test_body_at_an_odd_host_address_and_device_resident(ctx, name):
    """the body handed in at an odd host address, and through _dev from every device alignment: the same tables"""
    import torch
    c = sr.case(name)
    buf = np.zeros(len(c.body) + 9, np.uint8)
    for shift in (1, 3):
        view = buf[shift:shift + len(c.body)]
        view[:] = c.body
        assert view.ctypes.data % 2 == 1
        same(call(ctx, c, body=view), c.expected, (name, "host", shift))
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 3):
        d = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        d[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        out = ctx.spectra_dev(d.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, cap=c.cap, pairs=c.pairs, joint_cap=c.joint_cap)
        same(out, c.expected, (name, "dev", shift))


@pytest.mark.parametrize("mode,N,kind,cap,jc,pk", [(COUNT, 65, "scattered", 255, 63, "g+1"), (PA, 130, "reversed", 1, 1, "many"), (COUNT, 300, "none", 300, 110, "one"),
                                                   (PA, 9, "none", 2, 255, "g")])
def test_two_calls_into_the_callers_tables(ctx, mode, N, kind, cap, jc, pk):
    """one call, against two calls over a cut into tables of the caller's that hold 2^32 - 1 in every cell: an add carries into the
    high word, the cells no row reaches stay as they were"""
    import torch
    rows, kw, cut = 1500, 2, 389
    body = sr.spectra_body(77 + N, rows, N, kw, mode, "uniform", (cap, jc))
    cols, pairs = sr.make_cols(kind, N, 5), sr.make_pairs(pk, N, jc, 6)
    M, P = N if cols is None else len(cols), len(pairs)
    rb = dr.row_bytes(kw, N, mode)
    eh, ej = sr.spectra_expected_np(body, N, kw, mode, cols, cap, pairs, jc)
    same(ctx.spectra(body, rows, N, kw, mode, cols=cols, cap=cap, pairs=pairs, joint_cap=jc), (eh, ej), "one call")
    dev = torch.device("cuda:0")
    seed = 0xFFFFFFFF
    d_h = torch.full((M, cap + 2), seed, dtype=torch.int64, device=dev)
    d_j = torch.full((P, jc + 1, jc + 1), seed, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    args = dict(cols=cols, cap=cap, pairs=pairs, joint_cap=jc, hist_dev=d_h.data_ptr(), joint_dev=d_j.data_ptr())
    first = ctx.spectra(body[:cut * rb], cut, N, kw, mode, keep=True, **args)
    try:
        assert first.hist_dev() == d_h.data_ptr() and first.joint_dev() == d_j.data_ptr()
        second = ctx.spectra(body[cut * rb:], rows - cut, N, kw, mode, **args)
    finally:
        first.free()
    torch.cuda.synchronize()
    got_h, got_j = d_h.cpu().numpy().view(np.uint64), d_j.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_h, eh + np.uint64(seed)) and np.array_equal(got_j, ej + np.uint64(seed))
    assert np.array_equal(second.hist, got_h) and np.array_equal(second.joint, got_j)      # the tables as they stand
    assert (got_h >> np.uint64(32)).any() and (got_j >> np.uint64(32)).any()      # adds carried
    assert ((got_h == seed) == (eh == 0)).all() and ((got_j == seed) == (ej == 0)).all() and (ej == 0).any()      # the cells no row reaches stay
    # one table of the caller's, the other the result's own
    d_h.fill_(seed)
    torch.cuda.synchronize()
    out = ctx.spectra(body, rows, N, kw, mode, cols=cols, cap=cap, pairs=pairs, joint_cap=jc, hist_dev=d_h.data_ptr())
    assert np.array_equal(out.hist, eh + np.uint64(seed)) and np.array_equal(out.joint, ej)


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib
    H, J = lib.SPECTRA_HIST, lib.SPECTRA_JOINT

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, pairs=((0, 8), (3, 3)), P=None, c1=255, c2=63, flags=H | J, n_rows=0, hist=None, joint=None):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        pp = None if pairs is None else np.ascontiguousarray(pairs, np.uint32).reshape(-1)
        M = (0 if not flags & H else N if cc is None else len(cc)) if M is None else M
        P = (0 if pp is None else len(pp) // 2) if P is None else P
        for fn in (lib._lib.kmx_spectra_host, lib._lib.kmx_spectra_dev):
            t = lib.KmxSpectraTask(kw, mode, N, M, None, n_rows, None if cc is None else cc.ctypes.data, None if pp is None else pp.ctypes.data, P, c1, c2, flags, hist, joint)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, pairs, P, c1, c2, flags, n_rows, hist, joint)

    OK, INVAL, UNSUP = 0, -2, -5
    call(INVAL, flags=0, cols=None, pairs=None); call(INVAL, flags=4); call(INVAL, flags=H | J | 0x80000000)       # no flag; unknown bits
    call(INVAL, N=0, cols=None, pairs=None, flags=H)
    call(INVAL, M=0)                                                 # HIST with M = 0
    call(INVAL, N=2, cols=(0, 1, 0), pairs=None, flags=H)            # n_use > n_cols
    call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4))         # an index at N; a duplicate
    call(INVAL, cols=None, M=8)                                      # the identity with M != N
    call(INVAL, flags=J, M=3, cols=None); call(INVAL, flags=J, cols=(1,), M=0); call(INVAL, flags=J, cols=None, hist=0x1000)       # without HIST: n_use, cols, hist
    call(INVAL, P=0); call(INVAL, pairs=None, P=2)                   # JOINT with P = 0, with pairs NULL
    call(INVAL, pairs=((0, 9),)); call(INVAL, pairs=((9, 0),))       # a pair index at N
    call(INVAL, flags=H, P=2, pairs=None); call(INVAL, flags=H, P=0); call(INVAL, flags=H, pairs=None, joint=0x1000)       # without JOINT: n_pairs, pairs, joint
    for c1 in (0, 65536, 2 ** 32 - 1):
        call(INVAL, c1=c1)
    for c2 in (0, 256, 2 ** 32 - 1):
        call(INVAL, c2=c2)
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, mode=7)
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode); call(UNSUP, mode=mode, kw=0)
    call(UNSUP, N=2 ** 30, cols=None, pairs=None, flags=H, c1=1)     # a row of 8 + 2^32 bytes
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32 - 255, mode=PA)
    call(UNSUP, N=2 ** 14, cols=None, c1=65535)                      # 2^14 * 65537 entries: 8 GiB and more
    call(UNSUP, P=2 ** 14, c2=255)                                   # 2^14 * 2^16 entries (the pairs are not read before the limit)
    # what is valid is taken: no rows
    for flags in (H, J, H | J):
        cc, pp = np.array([4, 2, 1], np.uint32), np.array([0, 8, 3, 3], np.uint32)
        t = lib.KmxSpectraTask(1, COUNT, 9, 3 if flags & H else 0, None, 0, cc.ctypes.data if flags & H else None, pp.ctypes.data if flags & J else None,
                               2 if flags & J else 0, 5 if flags & H else 0, 3 if flags & J else 0, flags, None, None)
        res = C.c_void_p()
        assert lib._lib.kmx_spectra_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
        h, j = np.ones((3, 7), np.uint64), np.ones((2, 4, 4), np.uint64)
        assert lib._lib.kmx_spectra_result_copy_hist(res, h.ctypes.data, h.size) == (OK if flags & H else INVAL) and h.any() != bool(flags & H)      # n_rows = 0 adds nothing
        assert lib._lib.kmx_spectra_result_copy_joint(res, j.ctypes.data, j.size) == (OK if flags & J else INVAL) and j.any() != bool(flags & J)
        if flags & H:
            assert lib._lib.kmx_spectra_result_copy_hist(res, h.ctypes.data, h.size - 1) == INVAL
        assert bool(lib._lib.kmx_spectra_result_hist_dev(res)) == bool(flags & H) and bool(lib._lib.kmx_spectra_result_joint_dev(res)) == bool(flags & J)
        lib._lib.kmx_spectra_result_free(res)
    # the context stays usable
    c = sr.case(pick(lambda c: c.n_cols == 9 and c.n_rows > 0))
    same(ctx.spectra(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, cap=c.cap, pairs=c.pairs, joint_cap=c.joint_cap), c.expected, c.name)


# ---- the launch shapes KMX_SPECTRA_CUS and KMX_SPECTRA_GRID force ------------------------------------------------------------------
def launch_shape(n_rows, units, groups, cus, grid_cap, tile, hist_lds, joint_lds, pa):
    """the launcher's formulas (spectra.hip, spectra_queue) -> the items and the grid of each kernel"""
    def plan(side, round_to, lds, least=256):
        cap = min(min(cus * min(8, max(2, 160 * 1024 // max(lds, 1))), 1 << 16), grid_cap)
        runs = max(1, cap // side)
        run = max(least, -(-n_rows // runs))
        run = -(-run // round_to) * round_to
        items = -(-n_rows // run) * side
        return dict(items=items, grid=min(items, cap), run=run)

    return dict(hist=plan(-(-units // 64), 1, hist_lds, 4096 if pa else 256), joint=plan(groups, tile, joint_lds))


@pytest.mark.parametrize("mode,N,rows,kind,cap,jc,pk", [(COUNT, 300, 2100, "scattered", 255, 63, "many"), (PA, 2100, 2100, "none", 2, 2, "many"),
                                                        (COUNT, 40, 4200, "reversed", 256, 110, "g+1"), (PA, 4200, 2100, "scattered", 1, 1, "one")])
def test_launch_shapes(ctx, mode, N, rows, kind, cap, jc, pk, monkeypatch):
    """KMX_SPECTRA_CUS=1 and KMX_SPECTRA_GRID=1 / 3 (read per call): one workgroup that strides over every item, and a few; each shape
    against the reference and, byte for byte, against the same call with the knobs unset (many workgroups)"""
    kw = 1
    body = sr.spectra_body(1234 + N, rows, N, kw, mode, "uniform", (cap, jc))
    cols, pairs = sr.make_cols(kind, N, 9), sr.make_pairs(pk, N, jc, 10)
    exp = sr.spectra_expected_np(body, N, kw, mode, cols, cap, pairs, jc)
    pl = sr.joint_plan(pairs, jc, dr.row_bytes(kw, N, mode))
    units = N if mode == COUNT else (N + 7) // 8
    tile = min(256, 16384 // dr.row_bytes(kw, N, mode)) if pl["stream"] else 256
    lds = (256 * cap if mode == COUNT and cap <= sr.HIST_LDS_CAP else 0, (4 * pl["G"] * (jc + 1) ** 2 if pl["lds"] else 0) + (16384 if pl["stream"] else 0))
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.delenv("KMX_SPECTRA_CUS", raising=False); monkeypatch.delenv("KMX_SPECTRA_GRID", raising=False)
    args = dict(cols=cols, cap=cap, pairs=pairs, joint_cap=jc)
    base = ctx.spectra(body, rows, N, kw, mode, **args)
    same(base, exp, "knobs unset")
    free = launch_shape(rows, units, pl["n_groups"], n_cu, 1 << 16, tile, *lds, mode == PA)
    assert free["hist"]["grid"] > 1 and free["joint"]["grid"] > 1, free
    for env in (dict(KMX_SPECTRA_CUS="1"), dict(KMX_SPECTRA_GRID="1"), dict(KMX_SPECTRA_GRID="3"), dict(KMX_SPECTRA_CUS="1", KMX_SPECTRA_GRID="3")):
        shape = launch_shape(rows, units, pl["n_groups"], 1 if "KMX_SPECTRA_CUS" in env else n_cu, int(env.get("KMX_SPECTRA_GRID", 1 << 16)), tile, *lds, mode == PA)
        assert shape["hist"]["grid"] <= free["hist"]["grid"] and shape["joint"]["grid"] <= free["joint"]["grid"], (env, shape)
        if env.get("KMX_SPECTRA_GRID") == "1":      # one workgroup, and it takes several items
            assert shape["hist"]["grid"] == shape["joint"]["grid"] == 1 and shape["hist"]["items"] + shape["joint"]["items"] > 2, (env, shape)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.spectra(body, rows, N, kw, mode, **args)
        for k in env:
            monkeypatch.delenv(k)
        same(out, exp, env)
        assert out.hist.tobytes() == base.hist.tobytes() and out.joint.tobytes() == base.joint.tobytes()


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
    d = tmp_path_factory.mktemp("kmxspectra")
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


def restated(bodies, n, kw, rmode, cols, cap, pairs, jc):
    """the restatement on a run's bodies, summed over the partitions -> (hist, joint or None)"""
    parts = [sr.spectra_expected_np(b, n, kw, rmode, cols, cap, pairs, jc) for b in bodies]
    return sum(p[0] for p in parts), sum(p[1] for p in parts) if pairs is not None else None


def check_driver(r, tmp_path, ids, cap, hist, id_pairs, jc, joint, solid, k):
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "hist.tsv").read() == sr.hist_text(ids, cap, hist)
    again = ["spectra", "--from-tables", tmp_path / "hist.tsv"]
    if id_pairs:
        assert open(tmp_path / "joint.tsv").read() == sr.joint_text(id_pairs, jc, joint)
        again += ["--joint", tmp_path / "joint.tsv", "--solid", solid] + (["--kmer-size", k] if k else [])
    sr.check_report(r.stdout, ids, cap, hist, id_pairs, jc, joint, solid, k)
    # the tables read back give the same report
    a = kmx(*again)
    assert a.returncode == 0 and a.stdout == r.stdout, a.stderr


@pytest.mark.parametrize("mode", KINDS)
def test_driver_on_the_golden_samples(golden_runs, mode, tmp_path):
    """every way of naming pairs, --samples, caps below the counts of the run, --solid, --gpus 2, against spectra_ref applied to the
    run's matrices; the tables read back with --from-tables print the same report"""
    run = golden_runs["runs"][mode]
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, 4, 31)
    rows = sum(len(b) for b in bodies) // dr.row_bytes(kw, n, rmode)
    outs = ("--hist", tmp_path / "hist.tsv", "--joint", tmp_path / "joint.tsv")
    allp = [(0, 1), (0, 2), (1, 2)]
    hist, joint = restated(bodies, n, kw, rmode, None, 255, allp, 63)
    assert rows > 100 and int(hist[0][:256].sum()) == rows and joint[1][1:, 1:].sum() > 0 and joint[1][0, 1:].sum() > 0      # shared and exclusive rows
    if rmode == COUNT:
        assert hist[2][2] > 0      # counts of 2
    r = kmx("spectra", "--run", run, *outs, "--all-pairs", "-v")
    check_driver(r, tmp_path, IDS, 255, hist, [(IDS[x], IDS[y]) for x, y in allp], 63, joint, 1, 31)
    assert "3 of 3 samples, 3 pairs, 4 partitions" in r.stderr
    one = r.stdout
    r = kmx("spectra", "--run", run, *outs, "--all-pairs", "--gpus", 2)
    check_driver(r, tmp_path, IDS, 255, hist, [(IDS[x], IDS[y]) for x, y in allp], 63, joint, 1, 31)
    assert r.stdout == one
    # a list, --against a sample that is not listed, caps of 1: every count is "1 or more"
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D3\n\nD1\n")
    ag = [(1, 2), (1, 0)]
    hist, joint = restated(bodies, n, kw, rmode, [2, 0], 1, ag, 1)
    r = kmx("spectra", "--run", run, *outs, "--samples", tmp_path / "s.txt", "--against", "D2", "--cap", 1, "--joint-cap", 1, "--output", tmp_path / "report.tsv")
    assert r.stdout == ""
    r.stdout = open(tmp_path / "report.tsv").read()
    check_driver(r, tmp_path, ["D3", "D1"], 1, hist, [("D2", "D3"), ("D2", "D1")], 1, joint, 1, 31)
    # --pairs with x = y and a pair twice, --solid 2 at a cap of 2
    with open(tmp_path / "p.txt", "w") as f:
        f.write("D1 D3\n\nD2\tD2\nD1 D3\n")
    pp = [(0, 2), (1, 1), (0, 2)]
    hist, joint = restated(bodies, n, kw, rmode, None, 2, pp, 2)
    r = kmx("spectra", "--run", run, *outs, "--pairs", tmp_path / "p.txt", "--cap", 2, "--joint-cap", 2, "--solid", 2)
    check_driver(r, tmp_path, IDS, 2, hist, [("D1", "D3"), ("D2", "D2"), ("D1", "D3")], 2, joint, 2, 31)
    # no pairs: the samples' lines alone
    hist, _ = restated(bodies, n, kw, rmode, None, 255, None, 63)
    r = kmx("spectra", "--run", run, "--hist", tmp_path / "hist.tsv")
    check_driver(r, tmp_path, IDS, 255, hist, [], 63, None, 1, None)


def test_driver_row_runs_and_lz4(golden_runs, tmp_path):
    """a --cpr run gives what the plain run gives; --batch-mb 1 cuts every partition of a hand-made hash run (100 count columns, 3000
    rows a partition) into runs of 1285 rows, on one shard and on two; a hash run has no k-mer size: no quality"""
    run = golden_runs["runs"]["kmer:count:bin"]
    r = kmx(*golden_runs["base"], "--file", golden_runs["dir"] / "in.fof", "--run-dir", tmp_path / "lz", "--mode", "kmer:count:bin", "--cpr")
    assert r.returncode == 0, r.stderr
    outs = ("--hist", tmp_path / "hist.tsv", "--joint", tmp_path / "joint.tsv")
    bodies, n, kw, rmode = dr.read_run_bodies(run, "kmer:count:bin", 4, 31)
    hist, joint = restated(bodies, n, kw, rmode, None, 255, [(0, 1), (0, 2), (1, 2)], 63)
    check_driver(kmx("spectra", "--run", tmp_path / "lz", *outs, "--all-pairs"), tmp_path, IDS, 255, hist, [("D1", "D2"), ("D1", "D3"), ("D2", "D3")], 63, joint, 1, 31)
    # 1 MB: two runs in flight, 512 KB each -- rows of 8 + 4 * 100 bytes: 1285 rows a run, 3000 rows a partition
    ids = [f"S{j}" for j in range(100)]
    bodies = [sr.spectra_body(40 + p, 3000, 100, 1, COUNT, "uniform", (9, 5)) for p in range(3)]
    root = dr.write_run(tmp_path / "wide", "hash:count:bin", 31, ids, bodies, window=16)
    with open(tmp_path / "p.txt", "w") as f:
        f.write("".join(f"S{x} S{y}\n" for x, y in ((0, 99), (50, 50), (17, 3), (3, 17), (64, 65))))
    pp = [(0, 99), (50, 50), (17, 3), (3, 17), (64, 65)]
    hist, joint = restated(bodies, 100, 1, COUNT, None, 9, pp, 5)
    r = kmx("spectra", "--run", root, *outs, "--pairs", tmp_path / "p.txt", "--cap", 9, "--joint-cap", 5, "--solid", 3, "--batch-mb", 1, "-v")
    check_driver(r, tmp_path, ids, 9, hist, [(ids[x], ids[y]) for x, y in pp], 5, joint, 3, None)
    assert "runs of 1285 rows" in r.stderr
    r2 = kmx("spectra", "--run", root, *outs, "--pairs", tmp_path / "p.txt", "--cap", 9, "--joint-cap", 5, "--solid", 3, "--batch-mb", 1, "--gpus", 2)
    assert r2.returncode == 0 and r2.stdout == r.stdout
