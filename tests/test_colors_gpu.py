"""`kmx colors` on the MI355X against tests/colors_ref.py: the C ABI through kmtricks_amd.lib on the bodies of colors_ref.gpu_cases() --
ids, first rows, sizes and patterns compared bit for bit, the identities on every case --, the class structures that go wrong in a hash
table of whole rows, signatures cut to 0 and 3 bits, the launch shapes the knobs of colors.hip force, odd addresses, the limits, and the
driver on the golden samples.  Run with -m gpu."""
import ctypes as C
import os, struct, subprocess
import numpy as np
import pytest

import dist_ref as dr
import colors_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
GD = os.path.join(ROOT, "tests", "golden")
COUNT, PA = cr.MODE_COUNT, cr.MODE_PA
U32 = cr.U32


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(out, exp, what):
    n, ids, first, sizes, patterns = exp
    assert out.n_classes == n, f"{what}: {out.n_classes} classes, expected {n}"
    assert out.ids.dtype == np.uint32 and out.ids.tobytes() == ids.tobytes(), f"{what}: ids, first difference at row {np.flatnonzero(out.ids != ids)[:3].tolist()}"
    assert out.first.tobytes() == first.tobytes(), f"{what}: first\n{out.first[:10]}\n{first[:10]}"
    assert out.sizes.tobytes() == sizes.tobytes(), f"{what}: sizes\n{out.sizes[:10]}\n{sizes[:10]}"
    assert out.patterns.dtype == np.uint64 and out.patterns.shape == patterns.shape and out.patterns.tobytes() == patterns.tobytes(), f"{what}: patterns"


def identical(a, b):
    return (a.n_classes == b.n_classes and a.ids.tobytes() == b.ids.tobytes() and a.first.tobytes() == b.first.tobytes() and a.sizes.tobytes() == b.sizes.tobytes()
            and a.patterns.tobytes() == b.patterns.tobytes())


def algo_bytes(n_rows, rb, M, n_classes):
    W = (M + 63) // 64
    return n_rows * rb + 2 * n_rows * (8 * W + 8) + 4 * n_rows + n_classes * (8 + 8 * W)


def run_and_check(ctx, body, rows, N, kw, mode, cols, a, what):
    exp = cr.colors_expected_np(body, N, kw, mode, cols, a)
    out = ctx.colors(body, rows, N, kw, mode, cols=cols, min_abund=a)
    same(out, exp, what)
    M = N if cols is None else len(cols)
    cr.check_identities(out.n_classes, out.ids, out.first, out.sizes, out.patterns, rows, M, spectrum0=cr.pan_expected_np(body, N, kw, mode, cols, a)[0][0])
    return out


@pytest.mark.parametrize("name", [c.name for c in cr.gpu_cases()])
def test_case(ctx, name):
    """columns on both sides of a byte and of a pattern word (W = 1, 2, 3, 5, 17); rows on both sides of a wave's chunk and of a tile;
    one class, every row a class, a skewed table, two classes row by row, patterns that differ in the last listed column only; lists in
    every order; key widths, so that rows fall at every alignment; PA padding bits all set; counts of 2^32 - 1 with min_abund 1, 2,
    2^32 - 1.  The identities of the header on every result, the one against pan's spectrum included"""
    c = cr.case(name)
    for a, exp in c.expected.items():
        out = ctx.colors(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a)
        same(out, exp, f"{name} a={a}")
        assert out.algo_bytes == algo_bytes(c.n_rows, dr.row_bytes(c.key_words, c.n_cols, c.mode), c.n_use, exp[0])
        spec0 = cr.pan_expected_np(c.body, c.n_cols, c.key_words, c.mode, c.cols, a)[0][0]
        cr.check_identities(out.n_classes, out.ids, out.first, out.sizes, out.patterns, c.n_rows, c.n_use, spectrum0=spec0)


# ---- class structures made by hand -------------------------------------------------------------------------------------------------
def count_body(counts, kw=1, seed=0):
    counts = np.ascontiguousarray(counts, "<u4")
    keys = np.random.default_rng(seed).integers(0, 256, (len(counts), 8 * kw), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([keys, counts.view(np.uint8).reshape(len(counts), -1)], axis=1)).reshape(-1)


def pa_body(held, pad, kw=1, seed=0):
    """held bool [rows, N]; pad bool [rows, (-N) % 8]: the padding bits as given"""
    keys = np.random.default_rng(seed).integers(0, 256, (len(held), 8 * kw), dtype=np.uint8)
    pay = np.packbits(np.concatenate([held, pad], axis=1), axis=1, bitorder="little")
    return np.ascontiguousarray(np.concatenate([keys, pay], axis=1)).reshape(-1)


@pytest.mark.parametrize("N", [70, 203])
def test_rows_that_differ_where_it_does_not_count_are_one_class(ctx, N):
    """rows that differ only in unlisted columns, only in PA padding bits, only in count values on the same side of min_abund: ONE class;
    rows that differ only in the last word of the pattern: as many classes as there are values of it"""
    rng = np.random.default_rng(N)
    rows = 300
    listed = np.sort(rng.permutation(N)[:N - 9]).astype(np.uint32)
    unlisted = np.setdiff1d(np.arange(N), listed)
    base = rng.random(N) < 0.5
    # only unlisted columns differ (COUNT and PA)
    held = np.tile(base, (rows, 1)); held[:, unlisted] = rng.random((rows, len(unlisted))) < 0.5
    out = run_and_check(ctx, count_body(held * rng.integers(1, 9, (rows, N))), rows, N, 1, COUNT, listed, 1, "unlisted, count")
    assert out.n_classes == 1 and out.sizes.tolist() == [rows]
    out = run_and_check(ctx, pa_body(held, np.ones((rows, (-N) % 8), bool)), rows, N, 1, PA, listed, 1, "unlisted, pa")
    assert out.n_classes == 1
    # only PA padding bits differ
    pad = rng.random((rows, (-N) % 8)) < 0.5
    pad[0] = True; pad[1] = False
    out = run_and_check(ctx, pa_body(np.tile(base, (rows, 1)), pad, kw=3), rows, N, 3, PA, None, 1, "padding bits")
    assert out.n_classes == 1 and (-N) % 8 > 0
    # count values on the same side of a: present ones in [a, 2^32 - 1], absent ones in [0, a)
    for a in (2, 1000, U32):
        counts = np.where(base, rng.integers(a, 2 ** 32, (rows, N)), rng.integers(0, a, (rows, N)))
        counts[0, base] = U32; counts[1, base] = a; counts[2, ~base] = a - 1
        out = run_and_check(ctx, count_body(counts, kw=2), rows, N, 2, COUNT, None, a, f"same side of a = {a}")
        assert out.n_classes == 1
    # only the last word differs: the last N - 64 * (W - 1) ordinals take every value a few rows each
    tail = N - 64 * ((N - 1) // 64)
    held = np.tile(base, (rows, 1))
    values = rng.integers(0, 2 ** min(tail, 5), rows)
    held[:, N - tail:N - tail + min(tail, 5)] = (values[:, None] >> np.arange(min(tail, 5))) & 1
    for mode, body in ((COUNT, count_body(held * 3)), (PA, pa_body(held, np.ones((rows, (-N) % 8), bool)))):
        out = run_and_check(ctx, body, rows, N, 1, mode, None, 1, "last word")
        assert out.n_classes == len(set(values.tolist())) == 32 and (out.patterns[:, :-1] == out.patterns[0, :-1]).all()


@pytest.mark.parametrize("a", [1, 2, U32])
def test_counts_on_both_sides_of_min_abund(ctx, a):
    """counts drawn from {0, a - 1, a, 2^32 - 1}: which side of a a count lies on is all that reaches a pattern"""
    rng = np.random.default_rng(a % 1000)
    rows, N = 257, 67
    counts = rng.choice(np.array([0, a - 1, a, U32], np.uint64), (rows, N)).astype(np.uint32)
    out = run_and_check(ctx, count_body(counts, kw=1), rows, N, 1, COUNT, None, a, f"a = {a}")
    present = counts >= a
    assert out.n_classes == len({r.tobytes() for r in present})


# ---- signatures cut short: the word compare decides ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 3])
@pytest.mark.parametrize("mode,N,rows,structure,kind", [(COUNT, 130, 700, "skewed", "scattered"), (PA, 257, 300, "distinct", "none"), (COUNT, 8, 700, "random", "reversed"),
                                                        (PA, 64, 700, "alternate", "none"), (COUNT, 65, 255, "distinct", "reversed")])
def test_hash_bits(ctx, bits, mode, N, rows, structure, kind, monkeypatch):
    """KMX_COLORS_HASH_BITS keeps the low bits of every signature and SETS the others: different patterns share a signature, probe
    chains start at the table's end and wrap, inside a wave's group too.  Bodies of at most 300 classes and 700 rows (a condition of the
    test: chains are as long as the class count).  Equal to the reference and byte for byte to the same call with the knob unset"""
    cols = cr.make_cols(kind, N, 3)
    body = cr.structured_body(5000 + N, rows, N, 1, mode, structure, cols)
    exp = cr.colors_expected_np(body, N, 1, mode, cols)
    assert exp[0] <= 300 and rows <= 700, "the bound that keeps the chains short"
    monkeypatch.delenv("KMX_COLORS_HASH_BITS", raising=False)
    base = ctx.colors(body, rows, N, 1, mode, cols=cols)
    same(base, exp, "knob unset")
    monkeypatch.setenv("KMX_COLORS_HASH_BITS", str(bits))
    out = ctx.colors(body, rows, N, 1, mode, cols=cols)
    monkeypatch.delenv("KMX_COLORS_HASH_BITS")
    same(out, exp, f"hash bits {bits}")
    assert identical(out, base)
    assert exp[0] > 2 ** bits or structure == "alternate"      # more classes than signatures: patterns share one


# ---- the launch shapes KMX_COLORS_CUS and KMX_COLORS_GRID force ------------------------------------------------------------------
def launch_shape(n_rows, M, cus, grid_cap):
    """the launcher's formulas (colors.hip, colors_queue) -> trips of each stride loop"""
    W = (M + 63) // 64
    L = 1
    while L < 64 and L < M:
        L <<= 1
    RW = 64
    if L == 64:
        while RW > 4 and n_rows // RW < cus * 4 * 8:
            RW >>= 1
    chunks = (n_rows + RW - 1) // RW
    pack_grid = min((chunks + 3) // 4, min(min(cus * 8, 1 << 16), grid_cap))
    tiles = (n_rows + 255) // 256
    tile_grid = min(max(tiles, 1), grid_cap)
    gather_grid = min(max((n_rows * W + 255) // 256, 1), grid_cap)
    return dict(pack=-(-chunks // (4 * pack_grid)), tiles=-(-tiles // tile_grid), ids=-(-n_rows // (256 * tile_grid)), gather_bound=-(-(n_rows * W) // (256 * gather_grid)))


@pytest.mark.parametrize("mode,N,rows,kind,structure", [(COUNT, 300, 2100, "scattered", "distinct"), (PA, 1025, 2100, "none", "skewed"), (COUNT, 40, 4200, "reversed", "distinct"),
                                                        (PA, 64, 4200, "scattered", "random")])
def test_launch_shapes(ctx, mode, N, rows, kind, structure, monkeypatch):
    """KMX_COLORS_CUS=1 and KMX_COLORS_GRID=3 (read per call): several trips of every stride loop -- the pack's chunks, the tiles of
    claim / flag / number, the rows of ids, the elements of gather --; each shape against the reference and, byte for byte, against the
    same call with the knobs unset"""
    import torch
    cols = cr.make_cols(kind, N, 9)
    M = N if cols is None else len(cols)
    body = cr.structured_body(1234 + N, rows, N, 1, mode, structure, cols)
    exp = cr.colors_expected_np(body, N, 1, mode, cols)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for k in ("KMX_COLORS_CUS", "KMX_COLORS_GRID", "KMX_COLORS_HASH_BITS"):
        monkeypatch.delenv(k, raising=False)
    base = ctx.colors(body, rows, N, 1, mode, cols=cols)
    same(base, exp, "knobs unset")
    W = (M + 63) // 64
    for env in (dict(KMX_COLORS_CUS="1"), dict(KMX_COLORS_GRID="3"), dict(KMX_COLORS_CUS="1", KMX_COLORS_GRID="3")):
        shape = launch_shape(rows, M, 1 if "KMX_COLORS_CUS" in env else n_cu, 3 if "KMX_COLORS_GRID" in env else 1 << 16)
        assert shape["pack"] > 1, (env, shape)
        if "KMX_COLORS_GRID" in env:
            assert shape["tiles"] > 1 and shape["ids"] > 1, (env, shape)
            assert -(-(exp[0] * W) // (256 * 3)) > 1, "the gather makes more than one trip over the classes there are"
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.colors(body, rows, N, 1, mode, cols=cols)
        for k in env:
            monkeypatch.delenv(k)
        same(out, exp, env)
        assert identical(out, base)


ODD = ["c-65-scattered-r700-k4-alternate", "c-130-scattered-r4200-k1-skewed-long", "p-9-one-r4200-k2-last", "p-1025-none-r4200-k4-alternate", "c-7-scattered-r255-k2-random",
       "p-65-reversed-r4200-k1-distinct-long"]


@pytest.mark.parametrize("name", ODD)
def test_body_at_an_odd_host_address_and_device_resident(ctx, name):
    """the body handed in at an odd host address, and through _dev from every device alignment: the same result as _host"""
    import torch
    c = cr.case(name)
    a = next(iter(c.expected))
    exp = c.expected[a]
    buf = np.zeros(len(c.body) + 9, np.uint8)
    for shift in (1, 3):
        view = buf[shift:shift + len(c.body)]
        view[:] = c.body
        assert view.ctypes.data % 2 == 1
        same(ctx.colors(view, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a), exp, (name, "host", shift))
    host = ctx.colors(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a)
    dev = torch.device("cuda:0")
    for shift in (0, 1, 2, 3):
        d = torch.zeros(len(c.body) + 8, dtype=torch.uint8, device=dev)
        d[shift:shift + len(c.body)] = torch.from_numpy(np.array(c.body)).to(dev)
        torch.cuda.synchronize()
        r = ctx.colors_dev(d.data_ptr() + shift, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a, keep=True)
        try:
            out = r.output()
            same(out, exp, (name, "dev", shift))
            assert identical(out, host)
            # ids_dev is the device array the copy came from
            from kmtricks_amd import lib
            back = np.zeros(c.n_rows, np.uint32)
            assert lib._lib.kmx_copy_to_host(ctx._h, back.ctypes.data, r.ids_dev(), 4 * c.n_rows) == 0 and back.tobytes() == exp[1].tobytes()
        finally:
            r.free()


def test_limits_are_refused(ctx):
    from kmtricks_amd import lib

    def call(code, kw=1, mode=COUNT, N=9, cols=(4, 2, 1), M=None, a=1, flags=0, n_rows=0):
        cc = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        M = (N if cc is None else len(cc)) if M is None else M
        for fn in (lib._lib.kmx_colors_host, lib._lib.kmx_colors_dev):
            t = lib.KmxColorsTask(kw, mode, N, M, None, n_rows, None if cc is None else cc.ctypes.data, a, flags)
            res = C.c_void_p()
            assert fn(ctx._h, C.byref(t), C.byref(res)) == code and not res.value, (code, kw, mode, N, cols, M, a, flags, n_rows)

    OK, INVAL, UNSUP = 0, -2, -5
    call(INVAL, N=0, cols=None); call(INVAL, M=0)
    call(INVAL, N=2, cols=(0, 1, 0))                               # n_use > n_cols
    call(INVAL, cols=(4, 9, 1)); call(INVAL, cols=(4, 2, 4))       # an index at N; a duplicate
    call(INVAL, cols=None, M=8)                                    # the identity with M != N
    call(INVAL, kw=0); call(INVAL, kw=5); call(INVAL, kw=0, mode=PA)
    call(INVAL, mode=7)
    call(INVAL, a=0); call(INVAL, a=0, mode=PA); call(INVAL, a=2, mode=PA)
    call(INVAL, flags=1); call(INVAL, flags=0x80000000)
    call(INVAL, n_rows=5)                                          # rows without a pointer
    for mode in (lib.MODE_BF, lib.MODE_BFC, lib.MODE_BFT):
        call(UNSUP, mode=mode); call(UNSUP, mode=mode, kw=0)
    call(UNSUP, N=2 ** 30, cols=None)                              # a row of 8 + 2^32 bytes
    call(UNSUP, n_rows=2 ** 32); call(UNSUP, n_rows=2 ** 32 - 255, mode=PA)
    # scratch beyond what the pool can give: 2^32 - 256 rows of 17 pattern words are 4 x 10^9 x (16 x 17 + 52) bytes, over a terabyte
    call(UNSUP, N=1025, cols=None, n_rows=2 ** 32 - 256); call(UNSUP, N=1025, cols=None, n_rows=2 ** 32 - 256, mode=PA)
    # n_rows = 0 is a valid call with C = 0
    t = lib.KmxColorsTask(1, COUNT, 9, 3, None, 0, np.array([4, 2, 1], np.uint32).ctypes.data, 1, 0)
    res = C.c_void_p()
    assert lib._lib.kmx_colors_host(ctx._h, C.byref(t), C.byref(res)) == OK and res.value
    assert lib._lib.kmx_colors_result_n_classes(res) == 0 and lib._lib.kmx_colors_result_algo_bytes(res) == 0
    one = np.ones(4, np.uint32)
    for fn in (lib._lib.kmx_colors_result_copy_ids, lib._lib.kmx_colors_result_copy_first, lib._lib.kmx_colors_result_copy_sizes):
        assert fn(res, one.ctypes.data, 0) == OK and one.all()
    lib._lib.kmx_colors_result_free(res)
    # a destination that is too small is refused; the context stays usable
    c = cr.case("c-8-scattered-r700-k1-alternate")
    a = next(iter(c.expected))
    r = ctx.colors(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, min_abund=a, keep=True)
    small = np.zeros(c.n_rows, np.uint32)
    assert lib._lib.kmx_colors_result_copy_ids(r._h, small.ctypes.data, c.n_rows - 1) == INVAL
    assert lib._lib.kmx_colors_result_copy_first(r._h, small.ctypes.data, r.n_classes() - 1) == INVAL
    assert lib._lib.kmx_colors_result_copy_patterns(r._h, small.ctypes.data, r.n_classes() - 1) == INVAL
    same(r.output(), c.expected[a], c.name)
    r.free()


def test_kernel_times_with_profiling(ctx):
    from kmtricks_amd import lib
    c = cr.case("c-130-scattered-r4200-k1-skewed-long")
    lib._lib.kmx_set_profiling(ctx._h, 1)
    try:
        r = ctx.colors(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, keep=True)
        parts = r.kernel_parts_ms()
        assert r.kernel_ms() > 0 and all(p >= 0 for p in parts) and sum(parts) <= r.kernel_ms() * 1.01 + 0.01
        r.free()
    finally:
        lib._lib.kmx_set_profiling(ctx._h, 0)
    r = ctx.colors(c.body, c.n_rows, c.n_cols, c.key_words, c.mode, cols=c.cols, keep=True)
    assert r.kernel_ms() < 0 and r.kernel_parts_ms() == (-1.0, -1.0, -1.0)
    r.free()


# ---- the driver on the golden samples ------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


KINDS = ("kmer:count:bin", "kmer:pa:bin")
IDS = ["D1", "D2", "D3"]


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """`kmx pipeline --hard-min 1` over the two golden samples and a third made of slices of both, 4 partitions, with the fixture's
    repartition table: every k-mer of every sample is a row (the recipe of tests/test_pan_gpu.py)"""
    from test_oracle_goldens import repart_table
    d = tmp_path_factory.mktemp("kmxcolors")
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
    """the restatement on the run's bodies -> (merged table, the pattern of every row per partition, rows, the bodies' payload per partition)"""
    bodies, n, kw, rmode = dr.read_run_bodies(run, mode, 4, 31)
    parts = [cr.colors_expected_np(b, n, kw, rmode, cols, a) for b in bodies]
    table, row_patterns = cr.merged_table(parts)
    rows = sum(len(b) for b in bodies) // dr.row_bytes(kw, n, rmode)
    present = []
    for b in bodies:
        pay = dr.split_payload(b, n, kw, rmode)[:, list(range(n)) if cols is None else cols]
        present.append(pay >= a if rmode == COUNT else pay.astype(bool))
    return table, row_patterns, rows, present


def check_driver(r, ids_dir, ids, a, table, row_patterns, present, top=None):
    assert r.returncode == 0, r.stderr
    assert r.stdout == cr.colors_text(ids, a, table, top)
    # --ids: every row's pattern rebuilt from its id and the FULL table equals the row of the matrix
    full = cr.sorted_table(table, len(ids))
    expected_files = cr.ids_files(table, row_patterns, len(ids))
    for p, want in enumerate(expected_files):
        got = open(os.path.join(ids_dir, f"ids_{p}.u32"), "rb").read()
        assert got == want, p
        rank = np.frombuffer(got, "<u4")
        rebuilt = np.array([[c == "1" for c in cr.bits_text(full[k][0], len(ids))] for k in rank], bool).reshape(len(rank), len(ids))
        assert np.array_equal(rebuilt, present[p]), p
    assert not os.path.exists(os.path.join(ids_dir, f"ids_{len(expected_files)}.u32"))


@pytest.mark.parametrize("mode", KINDS)
def test_driver_on_the_golden_samples(golden_runs, mode, tmp_path):
    """with and without --samples (reordered), --min-abund 2, --top 5, --ids and --gpus 2, against colors_ref applied to the run's matrices"""
    run = golden_runs["runs"][mode]
    table, row_patterns, rows, present = restated(run, mode, None)
    assert rows > 100 and 3 <= len(table) <= 7 and sum(table.values()) == rows and (0,) not in table      # every row is some sample's
    r = kmx("colors", "--run", run, "--ids", tmp_path / "ids", "-v")
    check_driver(r, tmp_path / "ids", IDS, 1, table, row_patterns, present)
    assert "3 of 3 samples, 4 partitions" in r.stderr
    one = r.stdout
    r = kmx("colors", "--run", run, "--ids", tmp_path / "ids2", "--gpus", 2)
    check_driver(r, tmp_path / "ids2", IDS, 1, table, row_patterns, present)
    assert r.stdout == one
    r = kmx("colors", "--run", run, "--ids", tmp_path / "ids3", "--top", 2)
    check_driver(r, tmp_path / "ids3", IDS, 1, table, row_patterns, present, top=2)      # the ids carry the rank in the full table
    r = kmx("colors", "--run", run, "--ids", tmp_path / "ids5", "--top", 5)
    check_driver(r, tmp_path / "ids5", IDS, 1, table, row_patterns, present, top=5)
    with open(tmp_path / "s.txt", "w") as f:
        f.write("D3\n\nD1\n")
    table2, row_patterns2, rows2, present2 = restated(run, mode, [2, 0])
    r = kmx("colors", "--run", run, "--ids", tmp_path / "ids4", "--samples", tmp_path / "s.txt", "--output", tmp_path / "table.tsv")
    assert r.stdout == "" and rows2 == rows and (0,) in table2      # the rows of D2 alone hold none of the two
    r.stdout = open(tmp_path / "table.tsv").read()
    check_driver(r, tmp_path / "ids4", ["D3", "D1"], 1, table2, row_patterns2, present2)
    if mode == "kmer:count:bin":
        table3, row_patterns3, _, present3 = restated(run, mode, [2, 0], a=2)
        assert table3 != table2
        r = kmx("colors", "--run", run, "--ids", tmp_path / "ids6", "--samples", tmp_path / "s.txt", "--min-abund", 2)
        check_driver(r, tmp_path / "ids6", ["D3", "D1"], 2, table3, row_patterns3, present3)


def test_driver_row_runs_and_lz4(golden_runs, tmp_path):
    """a --cpr run gives what the plain run gives; --batch-mb 1 cuts every partition of a hand-made run (100 count columns, 3000 rows a
    partition) into runs of rows whose classes repeat across the cut, on one shard and on two"""
    run = golden_runs["runs"]["kmer:count:bin"]
    r = kmx(*golden_runs["base"], "--file", golden_runs["dir"] / "in.fof", "--run-dir", tmp_path / "lz", "--mode", "kmer:count:bin", "--cpr")
    assert r.returncode == 0, r.stderr
    table, row_patterns, rows, present = restated(run, "kmer:count:bin", None)
    check_driver(kmx("colors", "--run", tmp_path / "lz", "--ids", tmp_path / "ids"), tmp_path / "ids", IDS, 1, table, row_patterns, present)
    # 1 MB: two runs in flight, 512 KB each -- rows of 8 + 4 * 100 bytes + 16 * 2 + 52: 1065 rows a run, 3000 rows a partition
    ids = [f"S{j}" for j in range(100)]
    bodies = [cr.structured_body(40 + p, 3000, 100, 1, COUNT, "skewed") for p in range(3)]
    root = dr.write_run(tmp_path / "wide", "hash:count:bin", 31, ids, bodies, window=16)
    parts = [cr.colors_expected_np(b, 100, 1, COUNT) for b in bodies]
    table, row_patterns = cr.merged_table(parts)
    present = [dr.split_payload(b, 100, 1, COUNT) >= 1 for b in bodies]
    assert max(table.values()) > 3 * 1065 and len(table) > 500      # the two large classes are met by every run of rows of every partition
    r = kmx("colors", "--run", root, "--ids", tmp_path / "wide_ids", "--batch-mb", 1, "-v")
    check_driver(r, tmp_path / "wide_ids", ids, 1, table, row_patterns, present)
    assert "runs of 1065 rows" in r.stderr
    r2 = kmx("colors", "--run", root, "--ids", tmp_path / "wide_ids2", "--batch-mb", 1, "--gpus", 2)
    check_driver(r2, tmp_path / "wide_ids2", ids, 1, table, row_patterns, present)
    assert r2.stdout == r.stdout
