"""`kmx filter` without a GPU: the restatement tests/filter_ref.py on hand-written cases, the driver's refusals (all of them come
before the first GPU call), and the new entries in the binding and the header."""
import os, re, struct, subprocess
import numpy as np
import pytest

import filter_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
B63 = 1 << 63


def K(*v):
    return np.array(v, np.uint64).reshape(len(v), -1)


def run_ref(rows, key, counts, mode=fr.MODE_COUNT, n_cols=2):
    rows = np.asarray(rows, np.uint64)
    pl = (np.arange(len(rows) * n_cols, dtype=np.uint32).reshape(len(rows), n_cols) + 100).view(np.uint8).reshape(len(rows), 4 * n_cols) if mode == fr.MODE_COUNT \
        else (np.arange(len(rows), dtype=np.uint8).reshape(len(rows), 1) + 1)
    return fr.filter_expected(rows, pl, key, np.array(counts, np.uint32), mode), pl


def test_worked_example():
    (m, v, ak, ac), pl = run_ref(K(3, 5, 9, 12), K(1, 5, 9, 20), [4, 2, 7, 3])
    assert list(v) == [0, 2, 7, 0] and ak.reshape(-1).tolist() == [1, 20] and ac.tolist() == [4, 3]
    exp = b"".join(struct.pack("<Q", k) + pl[i].tobytes() + struct.pack("<I", c) for i, k, c in ((1, 5, 2), (2, 9, 7)))
    assert m == exp
    (m, v, ak, ac), pl = run_ref(K(3, 5, 9, 12), K(1, 5, 9, 20), [4, 2, 7, 3], fr.MODE_PA)
    assert list(v) == [0, 1, 1, 0] and ak.reshape(-1).tolist() == [1, 20]
    assert m == struct.pack("<Q", 5) + pl[1].tobytes() + struct.pack("<Q", 9) + pl[2].tobytes()      # PA rows are unchanged


def test_hand_written_cases():
    (m, v, ak, ac), _ = run_ref(K(3, 5, 9), np.zeros((0, 1), np.uint64), [])
    assert m == b"" and list(v) == [0, 0, 0] and len(ak) == 0
    (m, v, ak, ac), _ = run_ref(K(100, 200, 300), K(1, 2, 99), [1, 2, 3])                      # the key below the first row
    assert m == b"" and not v.any() and ak.reshape(-1).tolist() == [1, 2, 99] and ac.tolist() == [1, 2, 3]
    (m, v, ak, ac), _ = run_ref(K(100, 200, 300), K(301, 2 ** 64 - 1), [5, 6])                 # ... above the last
    assert m == b"" and not v.any() and ak.reshape(-1).tolist() == [301, 2 ** 64 - 1]
    rows = K(0, 1, B63 - 1, B63, 2 ** 64 - 1)
    (m, v, ak, ac), pl = run_ref(rows, rows, [9, 8, 7, 6, 2 ** 32 - 1])                        # key = rows
    assert list(v) == [9, 8, 7, 6, 2 ** 32 - 1] and len(ak) == 0 and len(m) == 5 * (8 + 8 + 4) and m[-4:] == b"\xff" * 4
    (m, v, ak, ac), _ = run_ref(K(42), K(42), [3])                                             # one row
    assert list(v) == [3] and len(m) == 20 and len(ak) == 0
    (m, v, ak, ac), _ = run_ref(K(42), K(41, 43), [3, 4])
    assert list(v) == [0] and m == b"" and ak.reshape(-1).tolist() == [41, 43]
    (m, v, ak, ac), _ = run_ref(np.zeros((0, 1), np.uint64), K(3, 5), [1, 2])                  # a matrix without rows: by the definition
    assert m == b"" and len(v) == 0 and ak.reshape(-1).tolist() == [3, 5]


@pytest.mark.parametrize("kw", [1, 2, 3, 4])
def test_keys_that_differ_in_one_high_bit(kw):
    top = [0] * (kw - 1)
    rows = K([5] + top, [5 | B63] + top)                     # bit 63 of the low word alone
    (m, v, ak, ac), _ = run_ref(rows, K([5 | B63] + top), [7])
    assert list(v) == [0, 7] and len(ak) == 0
    if kw > 1:                                               # the top word alone; a key that is smaller in its top word and larger below
        low = [2 ** 64 - 1] * (kw - 1)
        rows = K(low + [1], low + [B63], low + [B63 + 1])
        (m, v, ak, ac), _ = run_ref(rows, K([0] * (kw - 1) + [B63], low + [B63], low + [2]), [1, 2, 3])
        assert list(v) == [0, 2, 0]
        assert [tuple(int(x) for x in r) for r in ak] == [tuple(low + [2]), tuple([0] * (kw - 1) + [B63])] and ac.tolist() == [3, 1]


# ---- the driver's refusals ------------------------------------------------------------------------------------------------------
def kmx_filter(*args):
    return subprocess.run([KMX, "filter", *[str(a) for a in args]], capture_output=True, text=True)


def base_header(compressed=0):
    return struct.pack("<QIB", 0x736b636972746d6b, 0, compressed)


def write_run(d, matrices=("matrix_0.count",), k=31, m=10, parts=4):
    """an input run directory by hand: gatb.config, the repartition table and the named files under matrices/"""
    for s in ("matrices", "config_gatb", "repartition_gatb"):
        os.makedirs(d / s)
    cfg = bytearray(144); struct.pack_into("<QQ", cfg, 0, k, m); struct.pack_into("<I", cfg, 128, parts)
    (d / "config_gatb" / "gatb.config").write_bytes(bytes(cfg))
    t = (np.arange(4 ** m) % parts).astype(np.uint16)
    (d / "repartition_gatb" / "repartition.minimRepart").write_bytes(struct.pack("<HQH", parts, len(t), 1) + t.tobytes() + struct.pack("<BI", 0, 0x12345678))
    for name in matrices:
        if name.endswith(".count"):
            hdr = base_header() + struct.pack("<QIIIIII", 0x6b5f78697274616d, k, 1, 1, 2, 0, 0)
        elif name.endswith(".pa"):
            hdr = base_header() + struct.pack("<QIIIIII", 0x6b5f74616d6170, k, 1, 2, 1, 0, 0)
        else:
            hdr = base_header() + struct.pack("<QIIII", 0x685f78697274616d, 4, 2, 0, 0)
        (d / "matrices" / name).write_bytes(hdr)
    return d


def write_fof(path, n=1):
    fa = path.parent / "s.fasta"
    fa.write_text(">r\n" + "ACGT" * 20 + "\n")
    path.write_text("".join(f"S{i} : {fa}\n" for i in range(n)))
    return path


def refused(r, message):
    assert r.returncode != 0 and message in r.stderr, (r.returncode, r.stderr)


def test_refusals_come_before_the_gpu(tmp_path):
    run, fof = write_run(tmp_path / "run"), write_fof(tmp_path / "key.fof")
    refused(kmx_filter("--in-matrix", run, "--output", tmp_path / "o1"), "--key is required")
    refused(kmx_filter("--key", fof, "--output", tmp_path / "o1"), "--in-matrix is required")
    refused(kmx_filter("--in-matrix", run, "--key", fof), "--output is required")
    refused(kmx_filter("--in-matrix", run, "--key", write_fof(tmp_path / "two.fof", 2), "--output", tmp_path / "o1"),
            "Filtering with many samples is not yet implemented. Fof must contain only one sample.")
    refused(kmx_filter("--in-matrix", run, "--key", fof, "--output", tmp_path), "Directory already exists!")
    for bad in ("x", "m,x", "kmv", ""):
        refused(kmx_filter("--in-matrix", run, "--key", fof, "--output", tmp_path / "o1", "--out-types", bad), "--out-types")
    refused(kmx_filter("--in-matrix", run, "--key", fof, "--output", tmp_path / "o1", "--count-bytes", "3"), "--count-bytes must be 1, 2 or 4")
    refused(kmx_filter("--in-matrix", run, "--key", fof, "--output", tmp_path / "o1", "--nonsense"), "unknown option")
    assert not (tmp_path / "o1").exists()      # nothing was laid out by a refused call


def test_a_run_without_kmer_matrices_is_refused(tmp_path):
    fof = write_fof(tmp_path / "key.fof")
    msg = "No files found for these parameters"
    refused(kmx_filter("--in-matrix", write_run(tmp_path / "none", ()), "--key", fof, "--output", tmp_path / "o"), msg)
    # a hash matrix alone does not count; nor does a compressed matrix without --cpr-in, or a plain one with it
    refused(kmx_filter("--in-matrix", write_run(tmp_path / "hash", ("matrix_0.count_hash", "matrix_1.pa_hash")), "--key", fof, "--output", tmp_path / "o"), msg)
    refused(kmx_filter("--in-matrix", write_run(tmp_path / "lz", ("matrix_0.count.lz4",)), "--key", fof, "--output", tmp_path / "o"), msg)
    refused(kmx_filter("--in-matrix", tmp_path / "none", "--key", fof, "--output", tmp_path / "o", "--cpr-in"), msg)
    refused(kmx_filter("--in-matrix", write_run(tmp_path / "plain"), "--key", fof, "--output", tmp_path / "o", "--cpr-in"), msg)
    refused(kmx_filter("--in-matrix", tmp_path / "does-not-exist", "--key", fof, "--output", tmp_path / "o"), msg)
    assert not (tmp_path / "o").exists()


def test_binding_and_header_carry_the_filter():
    from kmtricks_amd import lib
    assert callable(lib.Context.filter) and callable(lib.Context.filter_dev)
    assert (lib.FILTER_M, lib.FILTER_V, lib.FILTER_K) == (1, 2, 4) and lib.filter_want("m,v") == 3 and lib.filter_want("kmv") == 7
    h = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for name in ("kmx_filter_dev", "kmx_filter_host", "kmx_filter_result_wait", "kmx_filter_result_rows", "kmx_filter_result_row_bytes",
                 "kmx_filter_result_body_dev", "kmx_filter_result_copy_body", "kmx_filter_result_copy_vector", "kmx_filter_result_absent",
                 "kmx_filter_result_copy_absent", "kmx_filter_result_kernel_ms", "kmx_filter_result_algo_bytes", "kmx_filter_result_free"):
        assert re.search(r"\b" + name + r"\s*\(", h), name
    assert "km::FilterTask" in h and "km::MatrixFilter" in h
    assert int(re.search(r"#define KMX_VERSION (\d+)", h).group(1)) == lib.KMX_VERSION      # (no struct that existed changed: the binding still loads)
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "filter.hip")).read()
    assert "rocprim" not in src.lower() and "hipcub" not in src.lower()
