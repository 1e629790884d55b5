"""CPU-only: `kmx assoc` without a device -- the header's worked example by both restatements, the two restatements against each other
on every body tests/test_assoc_gpu.py sends (bit for bit, stat and beta included), the ABI, the driver's refusals that come before
kmx_create, and the driver's design (`kmx assoc --design`) against numpy's least squares."""
import ctypes, os, re, subprocess

import numpy as np
import pytest

import assoc_ref as ar
import dist_ref as dr
from assoc_ref import MODE_COUNT, MODE_PA, U32, INF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")


def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


# ---- the header's worked example, as literals -------------------------------------------------------------------------------------
EX_ROWS = [(0, 0, 1, 1), (1, 1, 1, 1), (1, 0, 1, 0), (0, 0, 0, 1)]
EX_VECS = [(-2, 2), (-2, 2), (2, 2), (2, 2)]
EX_ALL = [(2, 4, 3.0, 1.0), (4, 0, 0.0, 0.0), (2, 0, 0.0, 0.0), (1, 2, 1.0, 2.0 / 3.0)]      # rec, s0, stat, beta


def example_body(mode):
    keys = np.arange(4 * 8, dtype=np.uint8).reshape(4, 8)
    held = np.array(EX_ROWS, bool)
    if mode == MODE_COUNT:
        pay = (held * np.array([[5, 1, 7, U32]], np.uint32)).astype("<u4").view(np.uint8).reshape(4, 16)
    else:
        pay = np.packbits(np.concatenate([held, np.ones((4, 4), bool)], axis=1), axis=1, bitorder="little")      # padding bits set
    return np.concatenate([keys, pay], axis=1).reshape(-1)


@pytest.mark.parametrize("mode", [MODE_COUNT, MODE_PA])
def test_header_example(mode):
    body = example_body(mode)
    rows = ar.assoc_rows_py(body, 4, 1, mode, EX_VECS, 2, 3.0, 0.25)
    assert rows == EX_ALL
    a = ar.assoc_rows_np(body, 4, 1, mode, EX_VECS, 2, 3.0, 0.25)
    assert [(int(r["rec"]), int(r["s0"]), float(r["stat"]), float(r["beta"])) for r in a] == EX_ALL
    kept = ar.assoc_expected_py(body, 4, 1, mode, EX_VECS, 2, 3.0, 0.25, 1.0)
    assert [k[4] for k in kept] == [0, 3]
    recs, out = ar.assoc_expected_np(body, 4, 1, mode, EX_VECS, 2, 3.0, 0.25, 1.0)
    rb = dr.row_bytes(1, 4, mode)
    assert list(recs["row"]) == [0, 3] and out == body.reshape(4, rb)[[0, 3]].tobytes()
    # the example as the header tells it is in include/kmx.h
    txt = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert "kmx_assoc_dev" in txt and "With threshold 1.0 rows 0 and 3 are kept, in that order." in txt


def test_the_binding_takes_the_example_to_the_library():
    """Context.assoc exists and is refused for want of a device only (no CPU fallback)"""
    import torch
    from kmtricks_amd import lib
    assert hasattr(lib.Context, "assoc") and hasattr(lib.Context, "assoc_dev") and hasattr(lib, "AssocResult") and hasattr(lib, "AssocOutput")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_assoc_gpu.py runs the example")
    with pytest.raises(lib.KmxError, match="no HIP device"):
        lib.Context(0)


# ---- the two roads on what the GPU test sends -------------------------------------------------------------------------------------
def test_sweep_covers_every_axis():
    cs = ar.gpu_cases()
    for mode in (MODE_COUNT, MODE_PA):
        mine = [c for c in cs if c.mode == mode]
        assert {c.n_cols for c in mine} >= set(ar.COLUMNS)
        assert {c.n_vec for c in mine} >= set(ar.V_CUTS) | set(ar.VECTORS)
        assert {c.key_words for c in mine} == {1, 2, 3, 4}
    assert {c.n_rows for c in cs} >= set(ar.ROWS)
    assert {c.abund for c in cs if c.mode == MODE_COUNT} == {1, 2, U32}
    assert {c.threshold for c in cs} >= {0.0, INF} and any(c._thr == "median" for c in cs)
    assert any(c.min_rec > c.max_rec for c in cs)                        # an empty window
    assert any(c.vmin == 0.0 for c in cs) and any(c.vmin == c.n_use + 1 for c in cs)
    kinds = {c.name.split("-")[2] for c in cs}
    assert kinds >= {"none", "subset", "one", "second"}
    # every step of the kernel's vector count has a case on either side
    steps = ar.VP_STEPS
    for lo, hi in zip(steps, steps[1:]):
        for mode in (MODE_COUNT, MODE_PA):
            vs = {c.n_vec for c in cs if c.mode == mode}
            assert lo in vs and lo + 1 in vs and hi in vs
    # the results are not all of a kind: rows kept and rows dropped in the same call, in many calls
    assert sum(0 < len(c.expected[0]) < c.n_rows for c in cs) >= 30


@pytest.mark.parametrize("c", ar.gpu_cases(), ids=lambda c: c.name)
def test_roads_agree(c):
    recs, body = c.expected
    py = ar.assoc_expected_py(c.body, c.n_cols, c.key_words, c.mode, c.vecs, c.frac_bits, c.gain, c.vmin, c.threshold, c.cols, c.abund, c.min_rec, c.max_rec)
    assert [p[4] for p in py] == list(recs["row"])
    assert [p[3] for p in py] == list(recs["rec"]) and [p[2] for p in py] == list(recs["s0"])
    assert ar.same_bits([p[0] for p in py], recs["stat"]) and ar.same_bits([p[1] for p in py], recs["beta"])
    rb = dr.row_bytes(c.key_words, c.n_cols, c.mode)
    assert len(body) == len(recs) * rb


def test_wrapping_cases_would_wrap_32_bits():
    """the +-2^30 tables: a 32-bit sum of the second present column already leaves int32"""
    for name in ("c-130-none-r65-k2-ones-pos2-wrap", "p-130-none-r65-k2-ones-neg2-wrap"):
        c = ar.case(name)
        a = c.all_rows
        assert (np.abs(a["s0"]) >= 2 ** 31).all() and (a["rec"] == 130).all()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    txt = open(os.path.join(ROOT, "include", "kmx.h")).read()
    declared = set(re.findall(r"\b(kmx_assoc_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert declared == set(lib.ASSOC_EXPORTS) and len(declared) == 13
    for s in declared:
        assert hasattr(so, s), s
    assert int(re.search(r"\} kmx_assoc_task;\s*/\* (\d+) bytes \*/", txt).group(1)) == ctypes.sizeof(lib.KmxAssocTask) == 96
    assert int(re.search(r"\} kmx_assoc_rec;\s*/\* (\d+) bytes \*/", txt).group(1)) == lib.ASSOC_REC.itemsize == ar.REC.itemsize == 32
    assert lib.ASSOC_REC == ar.REC


# ---- the driver: refusals before kmx_create ---------------------------------------------------------------------------------------
IDS = [f"S{i}" for i in range(8)]


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_cpu")
    body = dr.make_body(5, 40, 8, 1, MODE_COUNT)
    root = dr.write_run(d / "run", "kmer:count:bin", 31, IDS, [body])
    return d, root


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


def refused(r, word):
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (r.returncode, r.stdout[:200], r.stderr)
    assert word in r.stderr, r.stderr
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)


PHENO = "".join(f"S{i} {v}\n" for i, v in enumerate([0.5, 1.5, -2, 3, 0.25, 7, 1, 2]))
COVAR = "sample\tPC1\tPC2\n" + "".join(f"S{i}\t{a}\t{b}\n" for i, (a, b) in enumerate([(0.1, 0.3), (-0.2, 0.1), (0.4, -0.3), (0, 0.2), (1, 1), (-0.3, -0.5), (0.2, 0.2), (0.6, -0.1)]))


def test_driver_refusals(run_dir):
    d, root = run_dir
    ph = write(d / "ph", PHENO)
    cv = write(d / "cv", COVAR)
    refused(kmx("assoc", "--run", root, "--pheno", write(d / "p1", PHENO + "S9 1\n")), "S9 is not in")
    refused(kmx("assoc", "--run", root, "--pheno", write(d / "p2", PHENO + "S3 1\n")), "named twice")
    refused(kmx("assoc", "--run", root, "--pheno", write(d / "p3", PHENO.replace("1.5", "1.5x"))), "not a finite number")
    refused(kmx("assoc", "--run", root, "--pheno", write(d / "p4", PHENO.replace("1.5", "nan"))), "not a finite number")
    refused(kmx("assoc", "--run", root, "--groups", write(d / "g1", "S0 case\nS1 maybe\n")), "neither case nor control")
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", write(d / "c1", COVAR.replace("S4\t1\t1\n", ""))), "missing from")
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", write(d / "c2", COVAR + "S4\t1\t1\n")), "named twice")
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", write(d / "c3", COVAR.replace("0.6", "zz"))), "not a finite number")
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", write(d / "c4", COVAR + "S9\t1\t1\n")), "S9 is not in")
    refused(kmx("assoc", "--run", root, "--pheno", write(d / "p5", "".join(f"S{i} 2.5\n" for i in range(8)))), "constant")
    refused(kmx("assoc", "--run", root, "--groups", write(d / "g2", "".join(f"S{i} case\n" for i in range(8)))), "constant")
    refused(kmx("assoc", "--run", root, "--pheno", write(d / "p6", "S0 1\nS1 2\nS2 4\n"), "--covar", cv), "M - q must be at least 2")
    wide = "sample" + "".join(f"\tPC{j}" for j in range(32)) + "\n" + "".join(f"S{i}" + "".join(f"\t{(i * 7 + j * 3) % 11}" for j in range(32)) + "\n" for i in range(8))
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", write(d / "c5", wide)), "more than 31 covariate columns")
    dep = "sample\tA\tB\n" + "".join(f"S{i}\t{i}\t{2 * i + 3}\n" for i in range(8))      # B = 2 A + 3 x the intercept
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", write(d / "c6", dep)), "covariates are linearly dependent")
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--covar", cv, "--pcs", 3), "--pcs 3")
    refused(kmx("assoc", "--run", root), "one of --pheno and --groups")
    refused(kmx("assoc", "--pheno", ph), "--run, or --design with --fof")
    refused(kmx("assoc", "--run", root, "--pheno", ph, "--min-rec", 5, "--max-rec", 4), "leave no recurrence class")
    refused(kmx("assoc", "--run", str(d / "nowhere"), "--pheno", ph), "not a kmtricks runtime directory")
    # the device-free form refuses the same design errors
    fof = os.path.join(root, "kmtricks.fof")
    refused(kmx("assoc", "--design", d / "des", "--fof", fof, "--pheno", ph, "--covar", write(d / "c7", dep)), "covariates are linearly dependent")
    refused(kmx("assoc", "--design", d / "des", "--fof", fof, "--pheno", d / "p5"), "constant")


def test_a_good_run_gets_as_far_as_the_device(run_dir):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_assoc_gpu.py runs the driver")
    d, root = run_dir
    r = kmx("assoc", "--run", root, "--pheno", write(d / "ph_ok", PHENO), "--covar", write(d / "cv_ok", COVAR))
    assert r.returncode == 1 and "kmx_create" in r.stderr and r.stdout == "", r.stderr


# ---- the driver's design against numpy --------------------------------------------------------------------------------------------
def parse_design(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "# kmx assoc design"
    head = dict(ln.split("\t") for ln in lines[1:7])
    assert list(head) == ["F", "M", "q", "gain", "vmin", "ymax"]
    F, M, q = int(head["F"]), int(head["M"]), int(head["q"])
    assert lines[7].split("\t") == ["sample", "column"] + [f"v{j}" for j in range(q + 1)]
    cells = [ln.split("\t") for ln in lines[8:]]
    assert len(cells) == M and all(len(c) == q + 3 for c in cells)
    return dict(F=F, M=M, q=q, gain=float(head["gain"]), vmin=float(head["vmin"]), ymax=float(head["ymax"]), ids=[c[0] for c in cells],
                cols=[int(c[1]) for c in cells], vecs=np.array([[int(x) for x in c[2:]] for c in cells], np.int64))


@pytest.mark.parametrize("M,q", [(4, 1), (9, 1), (9, 3), (40, 1), (40, 3), (40, 11), (200, 1), (200, 3), (200, 11)])
def test_design_against_numpy(tmp_path, M, q):
    rng = np.random.default_rng(100 * M + q)
    N = M + 3                                      # three samples of the fof are not listed
    ids = [f"T{i}" for i in range(N)]
    fof = write(tmp_path / "fof", "".join(f"{s} : /nowhere/{s}.fa\n" for s in ids))
    listed = np.sort(rng.permutation(N)[:M])
    K = q - 1
    y = rng.normal(size=M) * 3 + 1 if (M + q) % 2 else (rng.random(M) < 0.5).astype(float)
    if len(set(y)) == 1:
        y[0] = 1 - y[0]
    cov = rng.normal(size=(M, K)) * rng.uniform(0.5, 4, K) + rng.uniform(-2, 2, K)
    C = np.concatenate([np.ones((M, 1)), cov], axis=1)
    assert np.linalg.cond(C / np.linalg.norm(C, axis=0)) <= 100
    order = rng.permutation(M)                     # the files name the samples in any order: the design is in fof order
    ph = write(tmp_path / "ph", "".join(f"{ids[listed[m]]}\t{float(y[m])!r}\n" for m in order))
    args = ["assoc", "--design", tmp_path / "des", "--fof", fof, "--pheno", ph]
    if K:
        extra = rng.normal(size=(M, 2))            # two more columns than --pcs takes
        cv = "sample" + "".join(f"\tPC{j + 1}" for j in range(K + 2)) + "\n"
        cv += "".join(ids[listed[m]] + "".join(f"\t{float(v)!r}" for v in list(cov[m]) + list(extra[m])) + "\n" for m in order[::-1])
        args += ["--covar", write(tmp_path / "cv", cv), "--pcs", K]
    r = kmx(*args)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    D = parse_design(tmp_path / "des")
    assert (D["F"], D["M"], D["q"]) == (30, M, q) and D["ids"] == [ids[i] for i in listed] and D["cols"] == list(listed)
    one = float(2 ** 30)
    # numpy: the residual by least squares, the basis by QR with every column's sign fixed (R's diagonal positive, as Gram-Schmidt's)
    res = y - C @ np.linalg.lstsq(C, y, rcond=None)[0]
    ymax = np.abs(res).max()
    assert abs(D["ymax"] - ymax) <= 1e-12 * ymax
    Qn, Rn = np.linalg.qr(C)
    Qn = Qn * np.sign(np.diag(Rn))
    v0 = D["vecs"][:, 0]
    assert np.abs(v0 - np.rint(res / ymax * one)).max() <= 1
    assert np.abs(D["vecs"][:, 1:] - np.rint(Qn * one)).max() <= 1
    # ... and the projectors, whichever basis: the integers' own against numpy's
    Qd = D["vecs"][:, 1:] / one
    assert np.abs(Qd @ Qd.T - Qn @ Qn.T).max() <= 4 * q * 2.0 ** -31
    # gain = (M - q) / syy, syy the exact sum of the squares of the integers of vector 0
    syy = sum(int(x) * int(x) for x in v0) / float(2 ** 60)
    assert abs(D["gain"] - (M - q) / syy) <= 1e-12 * D["gain"]
    d = 2.0 ** -31
    assert D["vmin"] == max(2.0 ** -10, q * (2 * M * np.sqrt(M) * d + M * M * d * d) + (q + 2) * M * 2.0 ** -50)
