"""`kmx combine` without a GPU: the restatement tests/combine_ref.py on the issue's worked example and hand-written cases, the host
path of the driver against that restatement, the new entries of the header / library / binding, and the refusals of
`kmx combine --gpus` -- all of which come before the first GPU call."""
import os, re, struct, subprocess, ctypes
import numpy as np
import pytest

import combine_ref as cr
import combine_runs as runs

ROOT = runs.ROOT
KMX = runs.KMX
B63 = 1 << 63


def K(*v):
    return np.array(v, np.uint64).reshape(len(v), -1)


def counts(rows, cb=4):
    a = np.array(rows, cr.COUNT_DTYPE[cb])
    return a.reshape(len(rows), -1).view(np.uint8)


def count_rows(body, kw, n):
    """a count body -> [(key value, [counts])]"""
    a = np.frombuffer(body, np.uint8).reshape(-1, 8 * kw + 4 * n)
    return [(cr._value(r[:8 * kw].view(np.uint64)), r[8 * kw:].view(np.uint32).tolist()) for r in a.copy()]


def pa_rows(body, kw, n):
    a = np.frombuffer(body, np.uint8).reshape(-1, 8 * kw + (n + 7) // 8)
    return [(cr._value(r[:8 * kw].view(np.uint64)), int.from_bytes(r[8 * kw:].tobytes(), "little")) for r in a.copy()]


def test_worked_example():
    blocks = [(K(3, 9), counts([[1, 2], [5, 6]]), 2, 4), (K(3, 4), counts([[7], [8]], 1), 1, 1)]
    body, n = cr.combine_expected(blocks, 1, cr.MODE_COUNT)
    assert n == 3 and count_rows(body, 1, 3) == [(3, [1, 2, 7]), (4, [0, 0, 8]), (9, [5, 6, 0])]
    assert body == b"".join(struct.pack("<QIII", k, *c) for k, c in ((3, (1, 2, 7)), (4, (0, 0, 8)), (9, (5, 6, 0))))
    body, n = cr.combine_expected(blocks, 1, cr.MODE_COUNT, drop_last=True)
    assert n == 2 and count_rows(body, 1, 3) == [(3, [1, 2, 7]), (4, [0, 0, 8])]


def test_empty_blocks_and_one_block():
    e = (np.zeros((0, 1), np.uint64), np.zeros((0, 8), np.uint8), 2, 4)
    assert cr.combine_expected([e], 1, cr.MODE_COUNT) == (b"", 0)
    assert cr.combine_expected([e, e, e], 1, cr.MODE_COUNT, True) == (b"", 0)
    one = (K(5, 7), counts([[1, 0xFFFF], [3, 4]], 2), 2, 2)
    body, n = cr.combine_expected([one], 1, cr.MODE_COUNT)      # one block: copied and widened
    assert count_rows(body, 1, 2) == [(5, [1, 0xFFFF]), (7, [3, 4])]
    body, n = cr.combine_expected([one], 1, cr.MODE_COUNT, True)      # ... and its last key is held by one block
    assert count_rows(body, 1, 2) == [(5, [1, 0xFFFF])]
    body, n = cr.combine_expected([e, one, e], 1, cr.MODE_COUNT)      # empty blocks keep their columns
    assert count_rows(body, 1, 6) == [(5, [0, 0, 1, 0xFFFF, 0, 0]), (7, [0, 0, 3, 4, 0, 0])]


def test_all_keys_shared_and_no_key_shared():
    a, b = (K(1, 2, 3), counts([[1], [2], [3]]), 1, 4), (K(1, 2, 3), counts([[4], [5], [6]]), 1, 4)
    assert count_rows(cr.combine_expected([a, b], 1, cr.MODE_COUNT)[0], 1, 2) == [(1, [1, 4]), (2, [2, 5]), (3, [3, 6])]
    assert cr.combine_expected([a, b], 1, cr.MODE_COUNT, True)[1] == 3      # the greatest key is held by two
    c = (K(10, 20, 30), counts([[4], [5], [6]]), 1, 4)
    assert count_rows(cr.combine_expected([c, a], 1, cr.MODE_COUNT)[0], 1, 2) == [(1, [0, 1]), (2, [0, 2]), (3, [0, 3]), (10, [4, 0]), (20, [5, 0]), (30, [6, 0])]


@pytest.mark.parametrize("drop", [False, True])
def test_the_greatest_key_held_by_one_block_and_by_two(drop):
    a, b, c = (K(1, 9), counts([[1], [2]]), 1, 4), (K(2, 9), counts([[3], [4]]), 1, 4), (K(2, 8), counts([[5], [6]]), 1, 4)
    two = count_rows(cr.combine_expected([a, b], 1, cr.MODE_COUNT, drop)[0], 1, 2)
    assert two == [(1, [1, 0]), (2, [0, 3]), (9, [2, 4])]      # held by two: written either way
    one = count_rows(cr.combine_expected([a, c], 1, cr.MODE_COUNT, drop)[0], 1, 2)
    assert one == [(1, [1, 0]), (2, [0, 5]), (8, [0, 6])] + ([] if drop else [(9, [2, 0])])


def test_pa_blocks_at_unaligned_offsets_with_dirty_padding():
    # blocks of 1, 7, 8 and 9 columns: pos = 0, 1, 8, 16; every padding bit of the inputs is set
    b1 = (K(5), np.array([[0xFF]], np.uint8), 1)                     # bit 0 = 1, padding 1111111
    b7 = (K(5, 6), np.array([[0x80 | 0x41], [0xFF]], np.uint8), 7)   # columns 0 and 6; all seven
    b8 = (K(6), np.array([[0xA5]], np.uint8), 8)
    b9 = (K(5), np.array([[0x0F, 0xFF]], np.uint8), 9)               # columns 0-3 and 8; padding 1111111
    body, n = cr.combine_expected([b1, b7, b8, b9], 1, cr.MODE_PA)
    exp5 = 1 | (0x41 << 1) | (0x10F << 16)
    exp6 = (0x7F << 1) | (0xA5 << 8)
    assert pa_rows(body, 1, 25) == [(5, exp5), (6, exp6)] and len(body) == 2 * (8 + 4)
    assert exp5 < 1 << 25 and exp6 < 1 << 25      # the output's own padding bits are 0
    # the same blocks in another order: pos = 0, 9, 10, 17
    body, n = cr.combine_expected([b9, b1, b7, b8], 1, cr.MODE_PA)
    assert pa_rows(body, 1, 25) == [(5, 0x10F | (1 << 9) | (0x41 << 10)), (6, (0x7F << 10) | (0xA5 << 17))]


def test_mixed_count_widths():
    a = (K(1, 2), counts([[0xFF], [7]], 1), 1, 1)
    b = (K(2, 3), counts([[0xFFFF, 2], [3, 4]], 2), 2, 2)
    c = (K(1, 3), counts([[0xFFFFFFFF], [9]], 4), 1, 4)
    assert count_rows(cr.combine_expected([a, b, c], 1, cr.MODE_COUNT)[0], 1, 4) == [(1, [0xFF, 0, 0, 0xFFFFFFFF]), (2, [7, 0xFFFF, 2, 0]), (3, [0, 3, 4, 9])]


def test_two_word_keys_where_only_the_high_word_differs():
    a = (K([7, 1], [7, B63]), counts([[1], [2]]), 1, 4)
    b = (K([7, 2], [7, B63], [0, B63 + 1]), counts([[3], [4], [5]]), 1, 4)
    rows = count_rows(cr.combine_expected([a, b], 2, cr.MODE_COUNT)[0], 2, 2)
    assert rows == [(7 | (1 << 64), [1, 0]), (7 | (2 << 64), [0, 3]), (7 | (B63 << 64), [2, 4]), ((B63 + 1) << 64, [0, 5])]
    # a key smaller in its high word and larger below sorts first
    c = (K([2 ** 64 - 1, 1], [0, 2]), counts([[1], [2]]), 1, 4)
    assert [k for k, _ in count_rows(cr.combine_expected([c], 2, cr.MODE_COUNT)[0], 2, 1)] == [(2 ** 64 - 1) | (1 << 64), 2 << 64]


def test_the_two_roads_agree():
    """the numpy road (for the blocks of the GPU test that are too long for the dictionary) against the dictionary: every key width and
    key shape, both modes, count widths 1, 2 and 4, empty blocks, shares 0 ... 1, drop_last with one holder and with two"""
    from synth import SHAPES
    for kw in (1, 2, 3, 4):
        for si, shape in enumerate(SHAPES):
            for mode in (cr.MODE_COUNT, cr.MODE_PA):
                blocks = cr.synth_case(10 * kw + si, [300, 0, 170, 40], [7, 2, 9, 1], kw, mode, share=(0.0, 0.5, 1.0)[(kw + si) % 3], shape=shape,
                                       count_bytes=[4, 4, 1, 2], extreme=True)
                for drop in (False, True):
                    assert cr.combine_expected_np(blocks, kw, mode, drop) == cr.combine_expected(blocks, kw, mode, drop), (kw, shape, mode, drop)
    for mode in (cr.MODE_COUNT, cr.MODE_PA):
        empty = cr.synth_case(1, [0, 0], [3, 9], 2, mode)
        assert cr.combine_expected_np(empty, 2, mode, True) == cr.combine_expected(empty, 2, mode, True) == (b"", 0)
        top = (K(1, 9), np.full((2, cr.payload_bytes(3, mode)), 0x5A, np.uint8), 3, 4)
        for other in (K(2, 9), K(2, 8)):      # the greatest key held by two blocks, and by one
            blocks = [top, (other, np.full((2, cr.payload_bytes(2, mode)), 0xC3, np.uint8), 2, 4)]
            for drop in (False, True):
                assert cr.combine_expected_np(blocks, 1, mode, drop) == cr.combine_expected(blocks, 1, mode, drop)


def test_span_case_is_what_it_says():
    """block A's ends enclose every key of block B; A shares half its other keys with B; both ascend strictly"""
    for kw in (1, 2, 3, 4):
        for n_b in (2048 // kw, 2048 // kw + 1):
            a, b = cr.span_case(kw, kw, cr.MODE_COUNT, n_b)
            va, vb = [cr._value(k) for k in a[0]], [cr._value(k) for k in b[0]]
            assert len(va) == 200 and len(vb) == n_b and va == sorted(set(va)) and vb == sorted(set(vb))
            assert va[0] < vb[0] and va[-1] > vb[-1] and len(set(va) & set(vb)) == 99


# ---- the host path of the driver against the restatement ------------------------------------------------------------------------
def make_runs(tmp_path, kind, P=3, seed=0):
    """three runs of 3, 11 and 6 columns over P partitions -> (fof path, blocks[run][partition], total columns)"""
    pa, hashed = kind.startswith("pa"), kind.endswith("hash")
    k = 31 if hashed or not pa else 40
    kw = 1 if hashed else (k + 31) // 32
    ncols = [3, 11, 6]
    per_part = [cr.synth_case(100 * seed + p, [40, 25, 30], ncols, kw, cr.MODE_PA if pa else cr.MODE_COUNT, share=0.5,
                              shape="low-word-only" if kw == 2 else "uniform", extreme=True) for p in range(P)]
    paths = []
    for r in range(3):
        root = str(tmp_path / f"run{r}"); paths.append(root)
        runs.write_run(root, kind, k, [per_part[p][r] for p in range(P)], [f"S{r}a", f"S{r}b"])
    fof = tmp_path / "runs.fof"; fof.write_text("\n".join(paths) + "\n")
    return fof, per_part, k, kw, sum(ncols)


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("kind", runs.KINDS)
def test_host_path_equals_the_restatement(tmp_path, kind, compat):
    fof, per_part, k, kw, total = make_runs(tmp_path, kind)
    out = str(tmp_path / "combined")
    r = subprocess.run([KMX, "combine", "--fof", str(fof), "--output", out] + (["--reference-compat"] if compat else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    mode = cr.MODE_PA if kind.startswith("pa") else cr.MODE_COUNT
    for p, blocks in enumerate(per_part):
        exp, n = cr.combine_expected(blocks, kw, mode, compat)
        raw = open(f"{out}/matrices/matrix_{p}.{kind}", "rb").read()
        assert raw[:runs.header_bytes(kind)] == runs.matrix_header(kind, k, total, 7, p)
        assert raw[runs.header_bytes(kind):] == exp and n > 40


def test_host_path_joins_count_files_of_every_width(tmp_path):
    """a run that still holds its count files brings each of them as a one-column block of 1-, 2- or 4-byte counts"""
    P, k = 2, 31
    per_part = [cr.synth_case(7 + p, [30, 20, 25, 35], [1, 1, 1, 4], 1, cr.MODE_COUNT, share=0.4, count_bytes=[1, 2, 4, 4], extreme=True) for p in range(P)]
    runs.write_count_run(str(tmp_path / "runA"), k, [[per_part[p][s] for p in range(P)] for s in range(3)], ["A0", "A1", "A2"])
    runs.write_run(str(tmp_path / "runB"), "count", k, [per_part[p][3] for p in range(P)], ["B0", "B1", "B2", "B3"])
    fof = tmp_path / "runs.fof"; fof.write_text(f"{tmp_path}/runA\n{tmp_path}/runB\n")
    out = str(tmp_path / "combined")
    r = subprocess.run([KMX, "combine", "--fof", str(fof), "--output", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for p in range(P):
        exp, _ = cr.combine_expected(per_part[p], 1, cr.MODE_COUNT)
        assert open(f"{out}/matrices/matrix_{p}.count", "rb").read()[45:] == exp


# ---- what fails without the feature ---------------------------------------------------------------------------------------------
COMBINE_API = ("kmx_combine_dev", "kmx_combine_host", "kmx_combine_result_wait", "kmx_combine_result_rows", "kmx_combine_result_row_bytes",
               "kmx_combine_result_body_bytes", "kmx_combine_result_algo_bytes", "kmx_combine_result_body_dev", "kmx_combine_result_copy_body",
               "kmx_combine_result_kernel_ms", "kmx_combine_result_free")


def test_header_library_and_binding_carry_the_combine():
    h = open(os.path.join(ROOT, "include", "kmx.h")).read()
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    for name in COMBINE_API:
        assert re.search(r"\b" + name + r"\s*\(", h), name
        assert hasattr(so, name), f"libkmx.so does not export {name}"
    assert re.search(r"#define KMX_COMBINE_DROP_LAST 1u", h) and "kmx_block" in h and "block_on_device" in h
    from kmtricks_amd import lib
    assert callable(lib.Context.combine) and callable(lib.Context.combine_dev) and lib.COMBINE_DROP_LAST == 1
    assert int(re.search(r"#define KMX_VERSION (\d+)", h).group(1)) == lib.KMX_VERSION == 2      # (additive: no struct that existed changed)
    assert ctypes.sizeof(lib.KmxBlock) == 24 and ctypes.sizeof(lib.KmxCombineTask) == 32
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "combine.hip")).read().lower()
    assert "rocprim" not in src and "hipcub" not in src      # (no library kernel)


def refused(r, *messages):
    assert r.returncode == 1, (r.returncode, r.stderr)
    for m in messages:
        assert m in r.stderr, r.stderr


def test_bad_gpu_options_are_refused(tmp_path):
    fof, _, _, _, _ = make_runs(tmp_path, "count", P=1)
    base = [KMX, "combine", "--fof", str(fof), "--output", str(tmp_path / "o")]
    refused(subprocess.run(base + ["--gpus", "0"], capture_output=True, text=True), "--gpus must be at least 1")
    refused(subprocess.run(base + ["--gpus", "x"], capture_output=True, text=True), "bad number for --gpus: x")
    refused(subprocess.run(base + ["--gpus", "1", "--combine-batch-mb", "0"], capture_output=True, text=True), "--combine-batch-mb must be at least 1")
    refused(subprocess.run(base + ["--gpus"], capture_output=True, text=True), "missing value for --gpus")
    refused(subprocess.run(base + ["--gpus", "17"], capture_output=True, text=True), "--gpus must be at most 16")
    assert not (tmp_path / "o").exists()      # nothing was laid out by a refused call


def test_more_than_64_files_of_a_partition_are_refused_before_any_device(tmp_path):
    """a run that still holds 65 count files: `--gpus 1` refuses it before a device is touched -- the same message on a machine
    without a GPU and on one with -- and the host path joins it"""
    k, n = 31, 65
    samples = [[(K(10 + s, 500), counts([[s + 1], [3]], 1), 1, 1)] for s in range(n)]
    ids = [f"S{s:02d}" for s in range(n)]
    runs.write_count_run(str(tmp_path / "runA"), k, samples, ids)
    fof = tmp_path / "runs.fof"; fof.write_text(f"{tmp_path}/runA\n")
    r = subprocess.run([KMX, "combine", "--fof", str(fof), "--output", str(tmp_path / "g"), "--gpus", "1"], capture_output=True, text=True)
    refused(r, "partition 0 has 65 files", "at most 64 files of a partition", "run without --gpus")
    assert "kmx_create" not in r.stderr and "HIP" not in r.stderr and not os.path.exists(tmp_path / "g" / "matrices" / "matrix_0.count")
    r = subprocess.run([KMX, "combine", "--fof", str(fof), "--output", str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exp, rows = cr.combine_expected([s[0] for s in samples], 1, cr.MODE_COUNT)
    assert rows == 66 and open(tmp_path / "h" / "matrices" / "matrix_0.count", "rb").read()[45:] == exp


def test_gpu_path_keeps_the_host_paths_refusals(tmp_path):
    """mode, repartition equality, 'not a kmtricks directory' and the shape mismatch come first with --gpus too"""
    fof, per_part, k, kw, total = make_runs(tmp_path, "count", P=2)
    base = [KMX, "combine", "--fof", str(fof), "--gpus", "1", "--output"]
    # a PA matrix among count matrices
    os.remove(tmp_path / "run2" / "matrices" / "matrix_1.count")
    b = per_part[1][2]
    open(tmp_path / "run2" / "matrices" / "matrix_1.pa", "wb").write(runs.matrix_header("pa", k, 6, 7, 1))
    refused(subprocess.run(base + [str(tmp_path / "o1")], capture_output=True, text=True), "matrix_1.pa: not a kmer count matrix like the first run's")
    open(tmp_path / "run1" / "repartition_gatb" / "repartition.minimRepart", "wb").write(b"another table")
    refused(subprocess.run(base + [str(tmp_path / "o2")], capture_output=True, text=True), "are not mergeable")
    os.remove(tmp_path / "run1" / "repartition_gatb" / "repartition.minimRepart")
    refused(subprocess.run(base + [str(tmp_path / "o3")], capture_output=True, text=True), "run1: not a kmtricks directory.")
    open(tmp_path / "run0" / "options.txt", "w").write("Options: mode=bf, count_format=hash\n")
    refused(subprocess.run(base + [str(tmp_path / "o4")], capture_output=True, text=True), "not supported by 'kmtricks combine'")
