"""`kmx combine` on the MI355X, byte for byte against tests/combine_ref.py (the definition restated with a dictionary): the C ABI
(kmx_combine_host / kmx_combine_dev through kmtricks_amd.lib) over key shapes, column counts, block counts and shares of shared
keys, KMX_COMBINE_DROP_LAST, device-resident inputs (torch tensors, merge and filter results), and the driver's --gpus path against
its host path.  Run with -m gpu."""
import itertools, os, re, subprocess
import numpy as np
import pytest

import combine_ref as cr
import combine_runs as runs
from synth import SHAPES, synth_lists

pytestmark = pytest.mark.gpu
ROOT, KMX = runs.ROOT, runs.KMX


@pytest.fixture(scope="module")
def ctx():
    from kmtricks_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(got, exp, what):
    if got != exp:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
        bad = np.nonzero(a != b)[0] if len(a) == len(b) else [min(len(a), len(b))]
        raise AssertionError(f"{what}: {len(a)} bytes, expected {len(b)}; differs at {len(bad)} bytes, first at {bad[:8]}")


def check(ctx, blocks, kw, mode, drop_last=False, what=""):
    exp, rows = cr.combine_expected(blocks, kw, mode, drop_last)
    out = ctx.combine([(cr.block_body(b[0], b[1]), b[2], b[3]) for b in blocks], kw, mode, drop_last)
    total = sum(b[2] for b in blocks)
    assert out.row_bytes == 8 * kw + cr.payload_bytes(total, mode), what
    assert out.rows == rows, (what, out.rows, rows)
    same(out.body, exp, what)
    assert out.algo_bytes == sum(len(b[0]) * (8 * kw + cr.payload_bytes(b[2], mode, b[3])) for b in blocks) + len(exp), what
    return out


@pytest.mark.parametrize("kw", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_key_shapes(ctx, kw, shape):
    """every key width over the five full-width shapes, count and PA, three blocks, counts at the maximum of their width"""
    for mode in (cr.MODE_COUNT, cr.MODE_PA):
        blocks = cr.synth_case(17 * kw + mode, [2500, 3000, 1800], [7, 200, 9], kw, mode, share=0.5, shape=shape, extreme=True)
        check(ctx, blocks, kw, mode, what=f"{shape} kw={kw} mode={mode}")


COLS = [1, 7, 8, 9, 200, 1000, 4096]


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
@pytest.mark.parametrize("cols", list(itertools.combinations(COLS, 2)) + [(1, 7, 8), (9, 200, 1), (4096, 1, 1000), (8, 8, 8), (7, 9, 4096), (1000, 200, 4096)])
def test_column_counts(ctx, cols, mode):
    """block columns in pairs and triples: rows from 12 bytes to 32 KB and more, PA offsets unaligned and aligned; both orders"""
    rows = [max(40, min(1500, 400000 // (sum(cols) * (4 if mode == cr.MODE_COUNT else 1))))] * len(cols)
    for order in (cols, cols[::-1]):
        blocks = cr.synth_case(sum(order) + len(order), rows, list(order), 1 + (sum(order) & 1), mode, share=0.4, extreme=True)
        check(ctx, blocks, 1 + (sum(order) & 1), mode, what=f"cols={order} mode={mode}")


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
@pytest.mark.parametrize("B", [1, 2, 5, 64])
def test_block_counts(ctx, B, mode):
    rng = np.random.default_rng(B)
    cols = [int(c) for c in rng.choice([1, 2, 3, 8, 13], B)]
    blocks = cr.synth_case(B, [int(r) for r in rng.integers(200, 900, B)], cols, 1, mode, share=0.6, extreme=True)
    check(ctx, blocks, 1, mode, what=f"B={B} mode={mode}")
    check(ctx, blocks, 1, mode, drop_last=True, what=f"B={B} mode={mode} drop_last")


def test_65_blocks_are_unsupported_and_nothing_runs(ctx):
    from kmtricks_amd import lib
    blocks = cr.synth_case(3, [10] * 65, [1] * 65, 1, cr.MODE_COUNT)
    with pytest.raises(lib.KmxError, match=r"\(-5\).*65 blocks, at most 64"):
        ctx.combine([(cr.block_body(b[0], b[1]), b[2], b[3]) for b in blocks], 1, cr.MODE_COUNT)
    with pytest.raises(lib.KmxError, match=r"\(-2\).*at least one block"):
        ctx.combine([], 1, cr.MODE_COUNT)
    with pytest.raises(lib.KmxError, match=r"\(-2\).*count_bytes must be 1, 2 or 4"):
        ctx.combine([(b"", 1, 3)], 1, cr.MODE_COUNT)
    with pytest.raises(lib.KmxError, match=r"\(-2\).*key_words"):
        ctx.combine([(b"", 1, 4)], 5, cr.MODE_COUNT)
    with pytest.raises(lib.KmxError, match=r"\(-5\).*Bloom"):
        ctx.combine([(b"", 1, 4)], 1, lib.MODE_BF)


@pytest.mark.parametrize("kw", [1, 2])
def test_count_files_of_every_width_beside_a_wide_matrix(ctx, kw):
    """one-column blocks of 1-, 2- and 4-byte counts (rows of 9, 10 and 12 bytes at kw = 1: nothing is aligned) around a wide block"""
    blocks = cr.synth_case(21 + kw, [3000, 2500, 700, 2800, 3100], [1, 1, 333, 1, 1], kw, cr.MODE_COUNT, share=0.5, count_bytes=[1, 2, 4, 4, 1], extreme=True)
    check(ctx, blocks, kw, cr.MODE_COUNT, what=f"mixed widths kw={kw}")
    check(ctx, blocks[::-1], kw, cr.MODE_COUNT, drop_last=True, what=f"mixed widths reversed kw={kw}")


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
@pytest.mark.parametrize("share", [0.0, 0.01, 0.5, 1.0])
def test_shared_keys_and_uneven_blocks(ctx, share, mode):
    """one block ten times longer than the others, one ten times shorter, empty blocks among them"""
    blocks = cr.synth_case(int(100 * share) + 5, [2000, 20000, 200, 0, 2000, 0], [5, 3, 11, 2, 70, 4], 1, mode, share=share, extreme=True)
    out = check(ctx, blocks, 1, mode, what=f"share={share} mode={mode}")
    assert out.rows == len({cr._value(k) for b in blocks for k in b[0]})
    if share == 1.0:
        assert out.rows == 20000


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
def test_empty_tasks(ctx, mode):
    for cols in ([3], [3, 9, 1]):
        blocks = cr.synth_case(1, [0] * len(cols), cols, 2, mode)
        for drop in (False, True):
            out = check(ctx, blocks, 2, mode, drop, what=f"empty {cols}")
            assert out.rows == 0 and out.body == b""


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("holders", [1, 2])
def test_drop_last(ctx, holders, drop, mode):
    """the greatest key of the union held by one block / by two, with and without the flag"""
    blocks = cr.synth_case(9, [700, 900, 500], [3, 9, 70], 1, mode, share=0.3, shape="near-max")
    top = max(max(cr._value(k) for k in b[0]) for b in blocks) + 5
    grown = []
    for i, (keys, pl, n, cb) in enumerate(blocks):
        if i in (0, 2)[:holders]:
            keys, pl = np.concatenate([keys, np.array([[top]], np.uint64)]), np.concatenate([pl, np.full((1, pl.shape[1]), 0x5A, np.uint8)])
        grown.append((keys, pl, n, cb))
    out = check(ctx, grown, 1, mode, drop, what=f"holders={holders} drop={drop} mode={mode}")
    distinct = len({cr._value(k) for b in grown for k in b[0]})
    assert out.rows == distinct - (1 if drop and holders == 1 else 0)


def test_dirty_pa_padding(ctx):
    """every padding bit of every input row set: none reaches the output, whose own padding bits are 0"""
    blocks = []
    for keys, pl, n, cb in cr.synth_case(77, [1500, 1200, 1400, 900], [1, 7, 9, 3], 1, cr.MODE_PA, share=0.6):
        pl = pl.copy()
        if n % 8:
            pl[:, -1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
        blocks.append((keys, pl, n, cb))
    out = check(ctx, blocks, 1, cr.MODE_PA, what="dirty padding")
    last = np.frombuffer(out.body, np.uint8).reshape(out.rows, out.row_bytes)[:, -1]
    assert not (last >> 4).any()      # 20 columns: the upper half of the third byte is padding


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
@pytest.mark.parametrize("kw", [1, 2, 3, 4])
def test_span_at_the_edge_of_the_staged_keys(ctx, kw, mode):
    """k_combine_rank stages a tile's span of another block's keys in LDS when it holds at most CAP = 2048 / kw keys: block A's one
    tile spans all of block B, of exactly CAP rows (staged) and of CAP + 1 (searched in global memory), in both block orders"""
    cap = 2048 // kw      # CB_LDS_W / KW (kmtricks_amd/csrc/combine.hip)
    for n_b in (cap, cap + 1):
        a, b = cr.span_case(100 * kw + n_b % 7 + mode, kw, mode, n_b)
        assert cr._value(a[0][0]) < cr._value(b[0][0]) and cr._value(a[0][-1]) > cr._value(b[0][-1]) and len(b[0]) == n_b
        for blocks in ([a, b], [b, a]):
            out = check(ctx, blocks, kw, mode, what=f"span={n_b} kw={kw} mode={mode} first={blocks[0][2]}")
            assert out.rows == 200 + n_b - 99


@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
def test_scan_carry(ctx, mode):
    """a block of more than 1024 rank tiles (262144 rows): k_combine_scan takes its tile counts in two trips of 1024 and carries the
    sum over; against the numpy road of the restatement (the dictionary is for a few thousand rows)"""
    rows = [262144 + 300, 1000]
    assert (rows[0] + 255) // 256 > 1024
    blocks = cr.synth_case(262 + mode, rows, [1, 3], 1, mode, share=0.5, extreme=True)
    for order in (blocks, blocks[::-1]):
        exp, n = cr.combine_expected_np(order, 1, mode)
        out = ctx.combine([(cr.block_body(b[0], b[1]), b[2], b[3]) for b in order], 1, mode)
        assert out.rows == n == rows[0] + 500
        same(out.body, exp, f"scan carry mode={mode} first={order[0][2]}")


def move_rows_log(orb):
    """rows of a workgroup of k_combine_move, as launch_combine_move works them out: about 128 KB of them"""
    sr_log = 8
    while sr_log > 0 and (orb << sr_log) > 131072:
        sr_log -= 1
    return sr_log


def test_output_rows_of_64_kb_and_more(ctx):
    """count rows so wide that a workgroup of k_combine_move takes two output rows at a time, and one (a row above 128 KB)"""
    seen = set()
    for cols in ([20000, 13000], [9000, 9000], [8000, 8000]):
        blocks = cr.synth_case(sum(cols) % 97, [40, 40], cols, 1, cr.MODE_COUNT, share=0.5, extreme=True)
        seen.add(move_rows_log(8 + 4 * sum(cols)))
        for order in (blocks, blocks[::-1]):
            check(ctx, order, 1, cr.MODE_COUNT, what=f"cols={[b[2] for b in order]}")
    assert seen == {0, 1} and move_rows_log(8 + 4 * 33000) == 0 and move_rows_log(8 + 4 * 16000) == 1


# ---- device residency -----------------------------------------------------------------------------------------------------------
def test_combine_dev_on_torch_tensors(ctx):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    for mode, kw in ((cr.MODE_COUNT, 1), (cr.MODE_PA, 2)):
        blocks = cr.synth_case(31 + mode, [4000, 3000, 5000], [1, 40, 9], kw, mode, share=0.5, count_bytes=[1, 4, 4], extreme=True)
        bodies = [cr.block_body(b[0], b[1]) for b in blocks]
        # one tensor, the blocks behind one another with a byte in front: no block is aligned
        flat = np.concatenate([np.zeros(1, np.uint8)] + [np.frombuffer(x, np.uint8) for x in bodies])
        t = torch.from_numpy(flat).to(dev)
        torch.cuda.synchronize()
        offs = np.concatenate([[1], 1 + np.cumsum([len(x) for x in bodies])])
        got = ctx.combine_dev([(t.data_ptr() + int(offs[i]), len(b[0]), b[2], b[3]) for i, b in enumerate(blocks)], kw, mode)
        host = ctx.combine([(bodies[i], b[2], b[3]) for i, b in enumerate(blocks)], kw, mode)
        exp, rows = cr.combine_expected(blocks, kw, mode)
        assert got.rows == host.rows == rows
        same(got.body, exp, f"combine_dev mode={mode}")
        same(host.body, exp, f"combine mode={mode}")


@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("mode", [cr.MODE_COUNT, cr.MODE_PA])
def test_combine_of_two_merges_equals_one_merge(ctx, mode, kw):
    """at recurrence-min 1 and share-min 0 the merge of 12 lists equals the combine of the merges of its first 5 and its last 7
    lists: the bodies of two kmx_merge_dev results are joined where they lie in HBM"""
    torch = pytest.importorskip("torch")
    from kmtricks_amd import lib
    N, rb = 12, 8 * kw + 4
    lists = synth_lists(500 + kw, N, 6000, 0.5, 300, kw=kw, key_bits=62 if kw == 1 else 100, count_max=9)
    soft = [1, 2, 3, 1, 4, 2, 1, 3, 5, 1, 2, 2]
    recs = [lib.pack_records(k, c, kw) for k, c in lists]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    dt = torch.from_numpy(np.concatenate(recs).view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    ptr = [(dt.data_ptr() + rb * int(offs[i]), int(offs[i + 1] - offs[i])) for i in range(N)]
    def merge(lo, hi):
        r = ctx.merge_dev([dict(lists=ptr[lo:hi], key_words=kw, soft_min=soft[lo:hi], rec_min=1, share_min=0, mode=mode)])
        r.wait()
        return r
    whole, a, b = merge(0, N), merge(0, 5), merge(5, N)
    try:
        assert a.rows() > 0 and b.rows() > 0 and whole.rows() > max(a.rows(), b.rows())
        got = ctx.combine_dev([(a.body_dev(), a.rows(), 5), (b.body_dev(), b.rows(), 7)], kw, mode)
        assert got.rows == whole.rows() and got.row_bytes == whole.row_bytes()
        same(got.body, whole.body(), f"merge identity mode={mode} kw={kw}")
    finally:
        for r in (whole, a, b):
            r.free()


def test_a_filter_result_is_a_block(ctx):
    import filter_ref as fr
    for mode in (cr.MODE_COUNT, cr.MODE_PA):
        row_keys, payload, key_keys, key_counts = fr.synth_case(5, 3000, 12, 1, mode, 0.5)
        other = cr.synth_case(6, [2000], [5], 1, mode, share=0.0)[0]
        torch = pytest.importorskip("torch")
        from kmtricks_amd import lib
        dev = torch.device("cuda", 0)
        rows_t = torch.from_numpy(np.frombuffer(fr.matrix_body(row_keys, payload), np.uint8).copy()).to(dev)
        key_t = torch.from_numpy(lib.pack_records(key_keys, key_counts, 1).view(np.int32).reshape(-1)).to(dev)
        oth_t = torch.from_numpy(np.frombuffer(cr.block_body(other[0], other[1]), np.uint8).copy()).to(dev)
        torch.cuda.synchronize()
        fres = ctx.filter_dev(rows_t.data_ptr(), len(row_keys), 12, 1, mode, (key_t.data_ptr(), len(key_counts)), "m", keep=True)
        try:
            n_f = 13 if mode == cr.MODE_COUNT else 12
            got = ctx.combine_dev([(oth_t.data_ptr(), len(other[0]), 5), (fres.body_dev(), fres.rows(), n_f)], 1, mode)
            em, _, _, _ = fr.filter_expected(row_keys, payload, key_keys, key_counts, mode)
            fk, fp = fr.split_body(em, 1, n_f, mode)
            exp, rows = cr.combine_expected([other, (fk, fp, n_f, 4)], 1, mode)
            assert fres.rows() > 0 and got.rows == rows
            same(got.body, exp, f"filter result as a block mode={mode}")
        finally:
            fres.free()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def make_runs(tmp_path, kind, P, rows, ncols, seed=0, cpr=False):
    pa, hashed = kind.startswith("pa"), kind.endswith("hash")
    k = 31 if hashed or not pa else 40
    kw = 1 if hashed else (k + 31) // 32
    per_part = [cr.synth_case(100 * seed + p, rows, ncols, kw, cr.MODE_PA if pa else cr.MODE_COUNT, share=0.5, extreme=True) for p in range(P)]
    paths = []
    for r in range(len(rows)):
        root = str(tmp_path / f"run{r}"); paths.append(root)
        runs.write_run(root, kind, k, [per_part[p][r] for p in range(P)], [f"S{r}a", f"S{r}b"])
    fof = tmp_path / "runs.fof"; fof.write_text("\n".join(paths) + "\n")
    return fof, per_part, kw


def kmx_combine(fof, out, *flags, timeout=300):
    r = subprocess.run([KMX, "combine", "--fof", str(fof), "--output", str(out), *flags], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r


def same_tree(a, b):
    ta, tb = runs.tree(a), runs.tree(b)
    assert sorted(ta) == sorted(tb)
    for name in ta:
        assert ta[name] == tb[name], name


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("kind", runs.KINDS)
def test_driver_on_one_gpu_equals_the_host_path(tmp_path, kind, compat):
    fof, per_part, kw = make_runs(tmp_path, kind, 5, [600, 400, 500], [3, 11, 6])
    flags = ["--reference-compat"] if compat else []
    kmx_combine(fof, tmp_path / "host", *flags)
    kmx_combine(fof, tmp_path / "gpu", "--gpus", "1", *flags)
    same_tree(tmp_path / "host", tmp_path / "gpu")
    mode = cr.MODE_PA if kind.startswith("pa") else cr.MODE_COUNT
    exp, _ = cr.combine_expected(per_part[2], kw, mode, compat)
    assert open(tmp_path / "gpu" / "matrices" / f"matrix_2.{kind}", "rb").read()[runs.header_bytes(kind):] == exp


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("kind", runs.KINDS)
def test_driver_with_two_shards_on_one_device(tmp_path, kind, compat):
    """two shards -- two host threads, each with its own context and upload buffers, writing at the same time -- on one device"""
    fof, _, _ = make_runs(tmp_path, kind, 7, [600, 400], [5, 9], seed=1)
    flags = ["--reference-compat"] if compat else []
    kmx_combine(fof, tmp_path / "host", *flags)
    kmx_combine(fof, tmp_path / "gpu2", "--gpus", "2", *flags)
    same_tree(tmp_path / "host", tmp_path / "gpu2")


def test_driver_compressed_in_and_out(tmp_path):
    """--cpr output, and that output (.lz4 matrices) as the input of a second combine: the same reader and writer as the host path"""
    fof, _, _ = make_runs(tmp_path, "count", 3, [500, 300], [4, 7], seed=2)
    kmx_combine(fof, tmp_path / "host", "--cpr")
    kmx_combine(fof, tmp_path / "gpu", "--gpus", "1", "--cpr")
    same_tree(tmp_path / "host", tmp_path / "gpu")
    assert os.path.exists(tmp_path / "gpu" / "matrices" / "matrix_0.count.lz4")
    fof2 = tmp_path / "again.fof"; fof2.write_text(f"{tmp_path}/gpu\n{tmp_path}/run0\n")
    kmx_combine(fof2, tmp_path / "host2")
    kmx_combine(fof2, tmp_path / "gpu2", "--gpus", "1")
    same_tree(tmp_path / "host2", tmp_path / "gpu2")


def test_driver_joins_count_files_of_every_width(tmp_path):
    P, k = 2, 31
    per_part = [cr.synth_case(7 + p, [300, 200, 250, 350], [1, 1, 1, 4], 1, cr.MODE_COUNT, share=0.4, count_bytes=[1, 2, 4, 4], extreme=True) for p in range(P)]
    runs.write_count_run(str(tmp_path / "runA"), k, [[per_part[p][s] for p in range(P)] for s in range(3)], ["A0", "A1", "A2"])
    runs.write_run(str(tmp_path / "runB"), "count", k, [per_part[p][3] for p in range(P)], ["B0", "B1", "B2", "B3"])
    for order in (("runA", "runB"), ("runB", "runA")):      # (the header comes from the last file: a count file's fields are shifted)
        fof = tmp_path / f"{order[0]}.fof"; fof.write_text("".join(f"{tmp_path}/{r}\n" for r in order))
        kmx_combine(fof, tmp_path / f"host_{order[0]}", "--reference-compat")
        kmx_combine(fof, tmp_path / f"gpu_{order[0]}", "--gpus", "1", "--reference-compat")
        same_tree(tmp_path / f"host_{order[0]}", tmp_path / f"gpu_{order[0]}")


def test_driver_in_key_ranges(tmp_path):
    """--combine-batch-mb so small that a partition is joined in several key ranges: the debug line says how many, the bytes are the
    host path's"""
    fof, _, _ = make_runs(tmp_path, "count", 2, [9000, 3000, 6000], [40, 25, 60], seed=3)
    kmx_combine(fof, tmp_path / "host", "--reference-compat")
    r = kmx_combine(fof, tmp_path / "gpu", "--gpus", "1", "--combine-batch-mb", "1", "--reference-compat", "-v", "debug")
    ranges = [int(x) for x in re.findall(r"\[kmx combine\] partition \d+: \d+ files, (\d+) key ranges", r.stderr)]
    assert len(ranges) == 2 and max(ranges) >= 3, r.stderr
    same_tree(tmp_path / "host", tmp_path / "gpu")
