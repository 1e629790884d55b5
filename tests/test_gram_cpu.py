"""`kmx pca` without a device: the two restatements of tests/gram_ref.py against each other and against the header's worked example, the
three identities against pan_ref and dist_ref, the sweep's coverage, the ABI's symbols and structure, every refusal of the driver that
comes before kmx_create, and `kmx pca --from-gram` -- the eigen-solve -- against numpy.linalg on matrices written here."""
import ctypes
import os, re, shutil, struct, subprocess
from fractions import Fraction

import numpy as np
import pytest

import dist_ref as dr
import gram_ref as gr
import pan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
COUNT, PA = gr.MODE_COUNT, gr.MODE_PA
U32 = gr.U32


def count_rows(rows, kw=1):
    return b"".join(bytes(8 * kw) + struct.pack(f"<{len(r)}I", *r) for r in rows)


def both(body, N, kw, mode, weights, cols=None, a=1):
    py = gr.gram_expected_py(body, N, kw, mode, weights, cols, a)
    npy = gr.gram_expected_np(body, N, kw, mode, weights, cols, a)
    assert [[int(x) for x in row] for row in npy] == py, (N, kw, mode, cols, a)
    return npy


def test_worked_example():
    """the example of include/kmx.h, as literals"""
    rows = [(1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1)]
    T = both(count_rows(rows), 3, 1, COUNT, [0, 6, 3, 0])
    assert T.tolist() == [[9, 3, 0], [3, 6, 3], [0, 3, 3]]
    pa = b"".join(bytes(8) + bytes([sum(bool(v) << i for i, v in enumerate(r)) | 0xF8]) for r in rows)      # every padding bit set
    assert both(pa, 3, 1, PA, [0, 6, 3, 0]).tolist() == [[9, 3, 0], [3, 6, 3], [0, 3, 3]]
    # a list: columns 2 and 0 -- row (1,1,0) has rec 1 over it, row (1,1,1) rec 2; column 1 is never touched
    assert both(count_rows(rows), 3, 1, COUNT, [0, 6, 3], cols=[2, 0]).tolist() == [[6 + 6 + 3, 0, 3], [0, 0, 0], [3, 0, 3 + 6]]
    # min_abund 2 on counts
    assert both(count_rows([(2, 1, 0), (2, 2, 0)]), 3, 1, COUNT, [0, 6, 3, 0], a=2).tolist() == [[9, 3, 0], [3, 3, 0], [0, 0, 0]]


@pytest.mark.parametrize("mode", [COUNT, PA])
def test_the_two_roads_agree_and_the_identities_hold(mode):
    """N 1 ... 130, lists of every kind, every padding bit set, counts of 2^32 - 1 with min_abund 1, 2 and 2^32 - 1, weights of every
    shape; the identities (a), (b), (c) of the header against pan_ref and dist_ref"""
    for N in range(1, 131):
        rows = max(5, 400 // N)
        kind = pr.KINDS[N % len(pr.KINDS)]
        cols = pr.make_cols(kind, N, N)
        M = N if cols is None else len(cols)
        a = gr.ABUNDS[N % 3] if mode == COUNT else 1
        body = dr.make_body(N, rows, N, 1 + N % 4, mode, fill=0.35, pad_ones=True, maxed=0.3, lo=1, hi=4)
        wkind = gr.WEIGHTS[N % len(gr.WEIGHTS)]
        w = gr.make_weights(wkind, M, N)
        T = both(body, N, 1 + N % 4, mode, w, cols, a)
        assert (T == T.T).all()
        listed = np.zeros(N, bool)
        listed[np.arange(N) if cols is None else cols] = True
        assert not T[~listed].any() and not T[:, ~listed].any()
        spec, sh = pr.pan_expected_np(body, N, 1 + N % 4, mode, cols, a)
        wi = [int(x) for x in w]
        for i in range(N):      # (a) and (c), in Python integers modulo 2^64
            assert int(T[i][i]) == sum(wi[R] * int(sh[R][i]) for R in range(M + 1)) % 2 ** 64
            assert sum(int(x) for x in T[i]) % 2 ** 64 == sum(R * wi[R] * int(sh[R][i]) for R in range(M + 1)) % 2 ** 64
        if a == 1:              # (b)
            inter, _ = dr.dist_expected_np(body, N, 1 + N % 4, mode)
            only = np.zeros_like(inter)
            only[np.ix_(listed, listed)] = inter[np.ix_(listed, listed)]
            assert np.array_equal(gr.gram_expected_np(body, N, 1 + N % 4, mode, gr.make_weights("dist", M), cols, 1), only)


def test_sums_wrap_modulo_2_64():
    rows = [(1, 1)] * 5
    w = [0, 0, U32]
    T = both(count_rows(rows), 2, 1, COUNT, w)
    assert T.tolist() == [[5 * U32] * 2] * 2 and 5 * U32 > 2 ** 32


def test_the_sweep_covers_what_it_says():
    cases = gr.gpu_cases()
    names = [c.name for c in cases]
    for N in gr.COLUMNS + [1025]:
        for m in "cp":
            assert any(n.startswith(f"{m}-{N}-") for n in names), (m, N)
    for rows in gr.ROWS:
        assert any(c.n_rows == rows for c in cases), rows
    for kw in (1, 2, 3, 4):
        assert any(c.key_words == kw and c.mode == mode for c in cases for mode in (COUNT, PA)), kw
    for word in gr.KINDS + gr.WEIGHTS + [str(s) for s in gr.SHAPES] + ["edge", "long"]:
        assert any(f"-{word}-" in n + "-" for n in names), word
    for a in gr.ABUNDS:
        assert any(c.abund == a and c.mode == COUNT for c in cases), a
    assert all(c.abund == 1 for c in cases if c.mode == PA)
    assert len(cases) < 80
    # the padding edge: classes of exactly 63, 64 and 65 rows
    c = gr.case(next(n for n in names if "-edge-" in n))
    sizes = gr.class_sizes(c.body, c.n_cols, c.key_words, c.mode, c.cols, c.abund)
    assert {63, 64, 65} <= set(int(x) for x in sizes)
    # cells pass 2^32 where every weight is 2^32 - 1
    c = gr.case(next(n for n in names if n.endswith("-long")))
    assert (c.expected >> np.uint64(32)).any()
    # some class of a weight of 0 has rows, the largest among them
    assert any(c.n_rows and not int(c.weights[c.n_use]) and gr.class_sizes(c.body, c.n_cols, c.key_words, c.mode, c.cols, c.abund)[c.n_use] for c in cases)


# ---- the driver's weights and Gram matrix, exact ----------------------------------------------------------------------------------
def test_driver_weights():
    # M = 4: M^2 / (R (M - R)) = 16/3, 4, 16/3; the largest F with 2^F 16/3 <= 2^32 - 1 is 29
    wt, F, used = gr.driver_weights(4, [7, 1, 2, 3, 9])
    assert F == 29 and wt == [0, round(Fraction(2 ** 29 * 16, 3)), 2 ** 31, round(Fraction(2 ** 29 * 16, 3)), 0] and used == 6
    # many rows: the sum of the weights must stay below 2^63
    wt, F, used = gr.driver_weights(4, [0, 2 ** 40, 0, 0, 0])
    assert F == 20 and wt[1] * 2 ** 40 < 2 ** 63 <= ((2 ** 22 * 16 + 3) // 6) * 2 ** 40
    assert gr.driver_weights(4, [0, 1, 1, 1, 0], scale="none") == ([0, 1, 1, 1, 0], 0, 3)
    assert gr.driver_weights(6, [1] * 7, min_rec=2, max_rec=3)[0][1] == 0 and gr.driver_weights(6, [1] * 7, min_rec=2, max_rec=3)[2] == 2
    # rounding is to nearest: (2^(F+1) M^2 + d) / (2 d)
    wt, F, _ = gr.driver_weights(3, [0, 1, 1, 0])
    assert wt[1] == wt[2] == round(Fraction(2 ** F * 9, 2)) and F == 29


def test_gram_exact_is_the_centred_weighted_gram():
    """G from the tables equals the definition row by row: the sum of w (x_i - p)(x_j - p) over the used rows, over n_used"""
    N, rows = 6, 40
    body = dr.make_body(3, rows, N, 1, PA, fill=0.5)
    present = gr.presence(body, N, 1, PA)
    spec, sh = pr.pan_expected_np(body, N, 1, PA)
    wt, F, used = gr.driver_weights(N, spec[0])
    T = gr.gram_expected_np(body, N, 1, PA, wt)
    G, mag = gr.gram_exact(N, None, wt, F, spec[0], sh, T)
    direct = [[Fraction(0)] * N for _ in range(N)]
    for x in present:
        R = int(x.sum())
        if wt[R]:
            w, p = Fraction(wt[R], 1 << F), Fraction(R, N)
            for i in range(N):
                for j in range(N):
                    direct[i][j] += w * (int(x[i]) - p) * (int(x[j]) - p)
    assert G == [[v / used for v in row] for row in direct]
    assert all(sum(row) == 0 for row in G)      # every row is centred: G 1 = 0
    assert all(mag[i][j] >= abs(G[i][j]) for i in range(N) for j in range(N))


# ---- header, binding, sources -----------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    declared = set(re.findall(r"\b(kmx_gram_\w+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "kmtricks_amd", "lib.py")).read()
    listed = re.search(r"GRAM_EXPORTS = \[(.*?)\]", src, re.S)
    assert listed, "kmtricks_amd/lib.py lists no GRAM_EXPORTS"
    bound = set(re.findall(r'"(kmx_gram_\w+)"', listed.group(1)))
    want = {"kmx_gram_dev", "kmx_gram_host"} | {"kmx_gram_result_" + s for s in ("wait", "table_dev", "copy_table", "kernel_ms", "kernel_parts_ms", "algo_bytes", "free")}
    assert declared == want == bound
    assert "kmx_gram_dev / _host" in hdr[:hdr.index("#ifndef KMX_H")]
    assert "/* ------------------------------------------------------------------- gram */" in hdr
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} kmx_gram_task;", hdr, re.S).group(1), flags=re.S)
    c_fields = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == ["key_words", "mode", "n_cols", "n_use", "rows", "n_rows", "cols", "weights", "min_abund", "flags", "table"]
    struct_src = re.search(r"class KmxGramTask\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S).group(1)
    assert c_fields == re.findall(r'\("(\w+)"', struct_src)
    for name in ("KmxGramTask", "GramResult", "GramOutput", "def gram(", "def gram_dev("):
        assert name in src, name
    for text in ("weights = (0, 6, 3, 0)", "(1,1,0)  rec 2, weight 3: T00, T01, T10, T11 += 3", "table = ((9,3,0),(3,6,3),(0,3,3))", "modulo 2^64"):
        assert text in hdr, text


def test_library_and_binding_structures():
    from kmtricks_amd import lib
    so = ctypes.CDLL(os.path.join(ROOT, "kmtricks_amd", "libkmx.so"))
    assert len(lib.GRAM_EXPORTS) == 9
    for name in lib.GRAM_EXPORTS:
        assert hasattr(so, name), name
    assert ctypes.sizeof(lib.KmxGramTask) == 64 and lib.KmxGramTask.cols.offset == 32 and lib.KmxGramTask.weights.offset == 40 and lib.KmxGramTask.table.offset == 56
    src = open(os.path.join(ROOT, "kmtricks_amd", "csrc", "gram.hip")).read()
    assert "static_assert(sizeof(kmx_gram_task) == 64" in src


def test_gram_hip_has_knobs_of_its_own():
    csrc = os.path.join(ROOT, "kmtricks_amd", "csrc")
    src = open(os.path.join(csrc, "gram.hip")).read()
    for word in ("kmx_plan_cus", "kmx_grid_cap", "KMX_PLAN_CUS", "KMX_MAX_GRID", "KMX_PAN_"):
        assert word not in src, word
    assert 'kmx_env_cus("KMX_GRAM_CUS", ctx)' in src and 'kmx_env_grid("KMX_GRAM_GRID", dflt)' in src
    assert "gram.hip" in open(os.path.join(csrc, "Makefile")).read()
    host = open(os.path.join(ROOT, "kmtricks_amd", "host", "Makefile")).read()
    assert "kmx_pca.cpp" in host and "kmx_pca_math.hpp" in host
    assert "hip" not in open(os.path.join(ROOT, "kmtricks_amd", "host", "kmx_pca_math.hpp")).read().lower()


# ---- `kmx pca --from-gram`: the eigen-solve ---------------------------------------------------------------------------------------------
def kmx(*args):
    return subprocess.run([KMX] + [str(a) for a in args], capture_output=True, text=True)


def sym(rng, M, rank=None):
    """a Gram-like matrix: B B^T / rows of centred columns, of the rank asked for"""
    B = rng.standard_normal((M, rank or 3 * M))
    B -= B.mean(axis=0)
    G = B @ B.T / B.shape[1]
    return (G + G.T) / 2


def matrices():
    rng = np.random.default_rng(2024)
    out = {}
    for M in (2, 3, 4, 5, 8, 13, 21, 40):
        out[f"full-{M}"] = sym(rng, M)
    out["rank2-12"] = sym(rng, 12, rank=2)                        # rank deficient: ten eigenvalues at rounding level
    Q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    rep = Q @ np.diag([5.0, 2.0, 2.0, 2.0, 1.0, 0.5, 0.5, 0.25, 0.0]) @ Q.T      # repeated eigenvalues
    out["repeated-9"] = (rep + rep.T) / 2
    out["diagonal-6"] = np.diag([3.0, 1.0, 4.0, 1.5, 9.0, 2.5])
    out["scaled-10"] = sym(rng, 10) * 1e-9                        # the size of a real G's entries does not matter
    return out


# numpy.linalg.eigh's own residual and eigenvalue spread, measured on these matrices (see measured_eigh below and DESIGN.md section 22):
# the driver may be 8 x as far off -- both solvers are backward stable, with constants that are low polynomials in M
EIGH_FACTOR = 8


def measured_eigh(G):
    """-> (residual, spread): max over k of ||G v - lambda v||_inf, and max |lambda_eigh - lambda_eigvalsh|, each over ||G||_2, floored at
    one unit of rounding times M (a measurement of exactly 0 says nothing about the constant)"""
    M = len(G)
    lam, V = np.linalg.eigh(G)
    norm = max(abs(lam).max(), np.finfo(float).tiny)
    res = max(np.abs(G @ V[:, k] - lam[k] * V[:, k]).max() for k in range(M)) / norm
    spread = np.abs(lam - np.linalg.eigvalsh(G, UPLO="U")).max() / norm
    floor = M * 2.0 ** -53
    return max(res, floor), max(spread, floor), norm


@pytest.mark.parametrize("name", list(matrices()))
def test_from_gram_against_numpy(name, tmp_path):
    G = matrices()[name]
    M = len(G)
    ids = [f"s{j}" for j in range(M)]
    with open(tmp_path / "g.tsv", "w") as f:
        f.write(gr.gram_text(ids, G))
    k = M - 1
    r = kmx("pca", "--from-gram", tmp_path / "g.tsv", "--pcs", k, "--evals", tmp_path / "ev.txt")
    assert r.returncode == 0, r.stderr
    got_ids, V = gr.parse_pcs(r.stdout)
    assert got_ids == ids and V.shape == (M, k)
    lam = np.array([float(x) for x in open(tmp_path / "ev.txt").read().split()])
    res, spread, norm = measured_eigh(G)
    print(f"{name}: eigh residual {res:.3e} spread {spread:.3e} (relative to ||G|| = {norm:.3e})")
    tol_res, tol_val = EIGH_FACTOR * res * norm, EIGH_FACTOR * spread * norm
    ref = np.linalg.eigvalsh(G)[::-1]
    assert len(lam) == M and (np.diff(lam) <= 0).all()      # all M, descending
    print(f"{name}: eigenvalue error {np.abs(lam - ref).max():.3e} (allowed {tol_val:.3e})")
    assert np.abs(lam - ref).max() <= tol_val
    # printed with 10 digits: a component is off by 5e-11 of its size at the most, on top of the solver's own error
    digits = 5e-10
    worst = 0.0
    for c in range(k):
        v = V[:, c]
        worst = max(worst, np.abs(G @ v - lam[c] * v).max())
        assert np.abs(G @ v - lam[c] * v).max() <= tol_res + digits * norm, (name, c)
        assert abs(np.linalg.norm(v) - 1) <= 8 * M * 2.0 ** -53 + digits, (name, c)
        big = np.abs(v).max()
        near = [i for i in range(M) if abs(v[i]) >= big * (1 - 1e-9)]
        assert any(v[i] > 0 for i in near) and (len(near) > 1 or v[near[0]] > 0), (name, c)
    print(f"{name}: worst residual {worst:.3e} (allowed {tol_res + digits * norm:.3e})")
    # pairwise orthogonal, also inside a repeated eigenvalue (Jacobi's vectors are a product of rotations)
    assert np.abs(V.T @ V - np.eye(k)).max() <= EIGH_FACTOR * max(res, spread) + 4 * digits
    # the default: min(10, M - 1) components; --output writes the same text
    r2 = kmx("pca", "--from-gram", tmp_path / "g.tsv", "--output", tmp_path / "pcs.tsv")
    assert r2.returncode == 0 and r2.stdout == ""
    ids2, V2 = gr.parse_pcs(open(tmp_path / "pcs.tsv").read())
    assert V2.shape == (M, min(10, M - 1)) and np.array_equal(V2, V[:, :min(10, M - 1)])


def test_pcs_text_is_pinned(tmp_path):
    with open(tmp_path / "g.tsv", "w") as f:
        f.write(gr.gram_text(["a", "b"], [[1.0, -1.0], [-1.0, 1.0]]))
    r = kmx("pca", "--from-gram", tmp_path / "g.tsv", "--evals", tmp_path / "ev.txt")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "sample\tPC1\na\t0.7071067812\nb\t-0.7071067812\n"
    assert open(tmp_path / "ev.txt").read() == "2\n0\n"


@pytest.mark.parametrize("edit,word", [
    (lambda t: t.replace("# samples: 3", "# samples: 4"), "id lines"),
    (lambda t: t.replace("# samples: 3\n", ""), "before the samples line"),
    (lambda t: t.replace("# samples: 3", "# samples: 1"), "outside [2, 32768]"),
    (lambda t: t.rsplit("\n", 2)[0] + "\n", "ends before row M"),
    (lambda t: t + "1\t2\t3\n", "more than M rows"),
    (lambda t: t.replace("1\t0.5\t0.25", "1\t0.5"), "fewer than M columns"),
    (lambda t: t.replace("1\t0.5\t0.25", "1\t0.5\t0.25\t7"), "more than M columns"),
    (lambda t: t.replace("0.5", "half", 1), "expected a finite number"),
    (lambda t: t.replace("0.5", "nan", 1), "expected a finite number"),
    (lambda t: t.replace("0.25\t0.5\t3", "0.25\t0.75\t3"), "not symmetric"),
    (lambda t: "", "ends before row M"),
])
def test_a_malformed_gram_is_refused(edit, word, tmp_path):
    text = gr.gram_text(["a", "b", "c"], [[1.0, 0.5, 0.25], [0.5, 2.0, 0.5], [0.25, 0.5, 3.0]])
    with open(tmp_path / "g.tsv", "w") as f:
        f.write(edit(text))
    r = kmx("pca", "--from-gram", tmp_path / "g.tsv", "--output", tmp_path / "out.tsv")
    assert r.returncode == 1 and "[error]" in r.stderr and word in r.stderr and r.stdout == "", r.stderr
    assert not os.path.exists(tmp_path / "out.tsv")
    with open(tmp_path / "g.tsv", "w") as f:
        f.write(text)
    for extra in (("--samples", "x"), ("--gpus", 2), ("--min-abund", 2), ("--gram", "y"), ("--scale", "none"), ("--run", "w"), ("--min-rec", 1), ("--pcs", 3), ("--pcs", 0)):
        r = kmx("pca", "--from-gram", tmp_path / "g.tsv", *extra)
        assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", extra
    assert kmx("pca", "--from-gram", tmp_path / "nothing.tsv").returncode == 1


# ---- the driver's refusals that need no device: each an [error] line, status 1, nothing on standard output, nothing written ---------------
MODES = ("kmer:count:bin", "kmer:pa:bin", "hash:count:bin", "hash:pa:bin")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmxpca")
    ids, k = ["A", "B", "C"], 31
    out = {}
    for mode in MODES:
        rmode = dr.KINDS[mode][5]
        bodies = [dr.make_body(p, 10, 3, 1, rmode) for p in range(2)]
        out[mode] = dr.write_run(d / mode.replace(":", "_"), mode, k, ids, bodies, window=16)
    return dict(dir=d, runs=out, ids=ids, k=k)


def refused(tmp_path, *args, word=None):
    outs = [tmp_path / n for n in ("out.tsv", "ev.txt", "gram.tsv")]
    r = kmx("pca", *args, "--output", outs[0], "--evals", outs[1], "--gram", outs[2])
    assert r.returncode == 1 and "[error]" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout[:200], r.stderr)
    assert word is None or word in r.stderr, (args, r.stderr)
    assert "kmx_create" not in r.stderr, r.stderr      # (without a device a refusal behind kmx_create would name it)
    assert not any(os.path.exists(p) for p in outs), "a refusal wrote a file"
    r = kmx("pca", *args)
    assert r.returncode == 1 and r.stdout == ""


def samples_file(tmp_path, text):
    with open(tmp_path / "s.txt", "w") as f:
        f.write(text)
    return tmp_path / "s.txt"


def test_usage_names_every_option():
    r = kmx("pca")
    assert r.returncode == 1 and r.stdout == ""
    for word in ("kmx pca --run", "--samples FILE", "--min-abund INT", "--scale eigenstrat|none", "--min-rec INT", "--max-rec INT", "--pcs INT=10", "--output FILE",
                 "--evals FILE", "--gram FILE", "--gpus INT", "--batch-mb INT", "kmx pca --from-gram FILE"):
        assert word in r.stderr, word


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_bad_options(runs, tmp_path, mode):
    run = runs["runs"][mode]
    refused(tmp_path, "--run", tmp_path / "nothing", word="not a kmtricks runtime directory")
    refused(tmp_path, "--run", run, "--frobnicate")
    refused(tmp_path, "--run", run, "--min-abund", 0, word="--min-abund")
    refused(tmp_path, "--run", run, "--min-abund", "-1", word="--min-abund")
    refused(tmp_path, "--run", run, "--min-abund", 2 ** 32, word="--min-abund")
    for g in (0, 17, "two"):
        refused(tmp_path, "--run", run, "--gpus", g, word="--gpus")
    refused(tmp_path, "--run", run, "--batch-mb", "lots", word="--batch-mb")
    refused(tmp_path, "--run", run, "--samples")
    refused(tmp_path, "--run", run, "--scale", "smartpca", word="--scale")
    for k in (0, 3, 10, "many"):      # three samples: 1 or 2 components
        refused(tmp_path, "--run", run, "--pcs", k, word="--pcs")
    refused(tmp_path, "--run", run, "--min-rec", 3, word="--min-rec")            # [3, 2] is empty
    refused(tmp_path, "--run", run, "--max-rec", 0, word="--max-rec")
    refused(tmp_path, "--run", run, "--min-rec", 2, "--max-rec", 1, word="leave no recurrence class")
    refused(tmp_path, "--run", run, "--samples", samples_file(tmp_path, "B\n"), word="at least 2 samples")
    refused(tmp_path, "--run", run, "--samples", samples_file(tmp_path, "B\nA\n"), "--pcs", 2, word="--pcs")
    if mode.split(":")[1] == "pa":
        refused(tmp_path, "--run", run, "--min-abund", 2, word="--min-abund")


@pytest.mark.parametrize("text,word", [
    ("A\nD\n", "D is not in the run"),           # an id that is not in the fof
    ("A\nB\nA\n", "A is named twice"),           # a duplicate
    ("A B\n", "expected one sample id"),         # two words
    ("", "names no sample"),                     # an empty list
    ("\n \n", "names no sample"),
])
def test_driver_refuses_bad_sample_lists(runs, tmp_path, text, word):
    for mode in ("kmer:count:bin", "hash:pa:bin"):
        refused(tmp_path, "--run", runs["runs"][mode], "--samples", samples_file(tmp_path, text), word=word)
    refused(tmp_path, "--run", runs["runs"]["kmer:pa:bin"], "--samples", tmp_path / "nothing.txt", word="nothing.txt")


def test_driver_refuses_modes_it_does_not_read(runs, tmp_path):
    body = dr.make_body(1, 4, 3, 1, COUNT)
    for said in ("hash:bf:bin", "hash:bfc:bin", "hash:bft:bin", "kmer:count:text", "kmer:pa:text", "hash:count:text"):
        root = dr.write_run(runs["dir"] / ("said_" + said.replace(":", "_")), "kmer:count:bin", 31, runs["ids"], [body], options_mode=said)
        refused(tmp_path, "--run", root, word=said)


@pytest.mark.parametrize("mode", MODES)
def test_driver_refuses_files_that_do_not_fit(runs, mode, tmp_path):
    ext, hdr, magic, cols_at, kw, rmode = dr.KINDS[mode]
    src = runs["runs"][mode]
    f1 = os.path.join("matrices", f"matrix_1.{ext}")

    def variant(name):
        shutil.copytree(src, tmp_path / name)
        return tmp_path / name

    d = variant("cut")           # a truncated body: no whole number of rows
    with open(d / f1, "r+b") as f:
        f.truncate(os.path.getsize(d / f1) - 1)
    refused(tmp_path, "--run", d, word=f"matrix_1.{ext}")
    d = variant("gone")          # a missing matrix
    os.remove(d / f1)
    refused(tmp_path, "--run", d, word=f"matrix_1.{ext}")
    d = variant("cols")          # a header of another number of columns than the fof has samples
    with open(d / f1, "r+b") as f:
        f.seek(cols_at); f.write(struct.pack("<I", 4))
    refused(tmp_path, "--run", d, word=f"matrix_1.{ext}")
    d = variant("magic")         # another kind of file under the name
    with open(d / f1, "r+b") as f:
        f.seek(13); f.write(struct.pack("<Q", 0x1234))
    refused(tmp_path, "--run", d, word="Invalid file format")
    d = variant("nofof")         # a fof with a sample more than the matrices have columns
    with open(d / "kmtricks.fof", "a") as f:
        f.write("D : /nowhere/D.fasta\n")
    refused(tmp_path, "--run", d, word=f"matrix_0.{ext}")
    d = variant("noopt")
    os.remove(d / "options.txt")
    refused(tmp_path, "--run", d, word="options.txt")
    d = variant("noparts")       # the partition count's file
    os.remove(d / ("repartition_gatb/repartition.minimRepart" if mode.startswith("kmer") else "hash.info"))
    refused(tmp_path, "--run", d)
