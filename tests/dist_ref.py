"""The definition of `kmx dist` (include/kmx.h, section "dist") restated for the tests, by two roads that share no code: plain Python
integers row by row (dist_expected_py) and numpy -- unpack, an int64 B.T @ B, np.minimum sums (dist_expected_np).  Beside them the
driver's two distance formulas and its text, readers for the matrix files of the five kinds of run the driver takes, and writers of a
run directory made by hand (what the driver's refusals are provoked on)."""
import os
import struct
import numpy as np

from kmfiles import KM_MAGIC

MODE_COUNT, MODE_PA, MODE_BF, MODE_BFC, MODE_BFT = 0, 1, 2, 3, 4
MATRIX_MAGIC, MATRIX_HASH_MAGIC = 0x6b5f78697274616d, 0x685f78697274616d
PA_MAGIC, PA_HASH_MAGIC, BITMATRIX_MAGIC = 0x6b5f74616d6170, 0x685f74616d6170, 0x74616d746962
# run mode -> (file extension, header bytes, magic, offset of the column count, key words (None: ceil(k / 32)), row mode)
KINDS = {"kmer:count:bin": ("count", 45, MATRIX_MAGIC, 33, None, MODE_COUNT), "kmer:pa:bin": ("pa", 45, PA_MAGIC, 29, None, MODE_PA),
         "hash:count:bin": ("count_hash", 37, MATRIX_HASH_MAGIC, 25, 1, MODE_COUNT), "hash:pa:bin": ("pa_hash", 37, PA_HASH_MAGIC, 21, 1, MODE_PA),
         "hash:bf:bin": ("cmbf", 49, BITMATRIX_MAGIC, 21, 0, MODE_BF)}


def row_bytes(key_words, n_cols, mode):
    return 8 * key_words + (4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8)


def as_bytes(body):
    return body if isinstance(body, (bytes, bytearray)) else np.ascontiguousarray(body, np.uint8).tobytes()


# ---- road 1: Python integers, row by row ------------------------------------------------------------------------------------------
def dist_expected_py(body, n_cols, key_words, mode, mins=False):
    """-> (inter, mins or None) as lists of lists of Python integers"""
    raw, rb, N = as_bytes(body), row_bytes(key_words, n_cols, mode), n_cols
    assert len(raw) % rb == 0
    inter = [[0] * N for _ in range(N)]
    mn = [[0] * N for _ in range(N)] if mins else None
    for r in range(len(raw) // rb):
        pay = raw[r * rb + 8 * key_words:(r + 1) * rb]
        if mode == MODE_COUNT:
            counts = struct.unpack(f"<{N}I", pay)
        else:
            bits = int.from_bytes(pay, "little")      # column i = bit i & 7 of byte i >> 3 = bit i of the little-endian integer
            counts = [(bits >> i) & 1 for i in range(N)]      # (the padding bits above N are never looked at)
        held = [i for i in range(N) if counts[i]]
        for i in held:
            row = inter[i]
            for j in held:
                row[j] += 1
        if mins:
            for i in held:
                row, ci = mn[i], counts[i]
                for j in held:
                    row[j] += ci if ci < counts[j] else counts[j]
    return inter, mn


# ---- road 2: numpy ------------------------------------------------------------------------------------------------------------------
def split_payload(body, n_cols, key_words, mode):
    """-> the rows' payload: uint32 [rows, N] counts, or bool [rows, N] bits"""
    rb = row_bytes(key_words, n_cols, mode)
    a = np.frombuffer(as_bytes(body), np.uint8).reshape(-1, rb)[:, 8 * key_words:]
    if mode == MODE_COUNT:
        return np.ascontiguousarray(a).view("<u4").reshape(len(a), n_cols)
    return np.unpackbits(a, axis=1, bitorder="little")[:, :n_cols].astype(bool)


def dist_expected_np(body, n_cols, key_words, mode, mins=False, blas=False):
    """-> (inter uint64 [N, N], mins uint64 [N, N] or None).  blas: the product in float64 (exact while a table entry is below 2^53:
    asserted) -- for the shapes of the bench and the stress script, where an integer product takes minutes"""
    pay = split_payload(body, n_cols, key_words, mode)
    B = pay != 0
    if blas:
        assert len(B) < 2 ** 53
        Bf = B.astype(np.float64)
        inter = (Bf.T @ Bf).astype(np.uint64)
    else:
        Bi = B.astype(np.int64)
        inter = (Bi.T @ Bi).astype(np.uint64)
    mn = None
    if mins:
        assert mode == MODE_COUNT
        C = pay.astype(np.uint64)
        mn = np.zeros((n_cols, n_cols), np.uint64)
        for i in range(n_cols):
            mn[i] = np.minimum(C[:, i:i + 1], C).sum(axis=0, dtype=np.uint64)
    return inter, mn


# ---- bodies ---------------------------------------------------------------------------------------------------------------------------
def make_body(seed, n_rows, n_cols, key_words, mode, fill=0.5, pad_ones=True, maxed=0.0, lo=1, hi=50):
    """n_rows rows of random keys (never read) and a payload in which a column is present with probability `fill`; PA / BF: every
    padding bit set (pad_ones); COUNT: counts in [lo, hi), a share `maxed` of the present ones 2^32 - 1.  -> uint8 array"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (n_rows, 8 * key_words), dtype=np.uint8)
    held = rng.random((n_rows, n_cols)) < fill
    if mode == MODE_COUNT:
        c = rng.integers(lo, hi, (n_rows, n_cols)).astype(np.uint32)
        if maxed:
            c[rng.random((n_rows, n_cols)) < maxed] = 0xFFFFFFFF
        c[~held] = 0
        pay = c.astype("<u4").view(np.uint8).reshape(n_rows, 4 * n_cols)
    else:
        pad = (-n_cols) % 8
        bits = np.concatenate([held, np.full((n_rows, pad), bool(pad_ones))], axis=1)
        pay = np.packbits(bits, axis=1, bitorder="little")
    return np.ascontiguousarray(np.concatenate([keys, pay], axis=1)).reshape(-1)


# ---- the driver's distances and text ------------------------------------------------------------------------------------------------
def jaccard(inter, i, j):
    ij, den = int(inter[i][j]), int(inter[i][i]) + int(inter[j][j]) - int(inter[i][j])
    return 1.0 - float(ij) / float(den) if den else 0.0


def braycurtis(mins, i, j):
    ij, den = int(mins[i][j]), int(mins[i][i]) + int(mins[j][j])
    return 1.0 - 2.0 * float(ij) / float(den) if den else 0.0


def format_table(ids, metric, inter, mins=None):
    """the text `kmx dist --metric <metric>` writes"""
    n = len(ids)
    lines = ["".join("\t" + s for s in ids)]
    for i in range(n):
        if metric == "shared":
            cells = [str(int(inter[i][j])) for j in range(n)]
        elif metric == "jaccard":
            cells = ["%.6f" % jaccard(inter, i, j) for j in range(n)]
        else:
            cells = ["%.6f" % braycurtis(mins, i, j) for j in range(n)]
        lines.append("\t".join([ids[i]] + cells))
    return "\n".join(lines) + "\n"


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def read_run_bodies(run, mode, n_parts, k):
    """the plain (not lz4) matrix bodies of a run made with `mode` -> (bodies, n_cols, key_words, row mode)"""
    ext, hdr, magic, cols_at, kw, rmode = KINDS[mode]
    kw = (k + 31) // 32 if kw is None else kw
    bodies, n = [], None
    for p in range(n_parts):
        raw = open(os.path.join(str(run), "matrices", f"matrix_{p}.{ext}"), "rb").read()
        m0, _, cpr, kind = struct.unpack_from("<QIBQ", raw, 0)
        assert m0 == KM_MAGIC and cpr == 0 and kind == magic, (p, mode)
        cols = struct.unpack_from("<I", raw, cols_at)[0]
        assert n in (None, cols)
        n = cols
        body = np.frombuffer(raw[hdr:], np.uint8)
        assert len(body) % row_bytes(kw, n, rmode) == 0
        bodies.append(body)
    return bodies, n, kw, rmode


def matrix_header(mode, k, n_cols, part, window=0):
    """the header `kmx pipeline` writes in front of a partition's matrix of a run made with `mode`"""
    base = struct.pack("<QIB", KM_MAGIC, 0, 0)
    kw = (k + 31) // 32
    if mode == "kmer:count:bin":
        return base + struct.pack("<QIIIIII", MATRIX_MAGIC, k, kw, 1, n_cols, 0, part)
    if mode == "kmer:pa:bin":
        return base + struct.pack("<QIIIIII", PA_MAGIC, k, kw, n_cols, (n_cols + 7) // 8, 0, part)
    if mode == "hash:count:bin":
        return base + struct.pack("<QIIII", MATRIX_HASH_MAGIC, 4, n_cols, 0, part)
    if mode == "hash:pa:bin":
        return base + struct.pack("<QIIII", PA_HASH_MAGIC, n_cols, (n_cols + 7) // 8, 0, part)
    assert mode == "hash:bf:bin"
    return base + struct.pack("<QIQQII", BITMATRIX_MAGIC, n_cols, window * part, window, 0, part)


def write_run(root, mode, k, ids, bodies, window=0, options_mode=None):
    """a run directory by hand: kmtricks.fof, options.txt, the partition count where the driver looks for it (the repartition table of a
    kmer run, hash.info of a hash run) and one matrix file a body.  options_mode: what options.txt says instead of `mode`"""
    root = str(root)
    os.makedirs(os.path.join(root, "matrices"), exist_ok=True)
    os.makedirs(os.path.join(root, "repartition_gatb"), exist_ok=True)
    with open(os.path.join(root, "kmtricks.fof"), "w") as f:
        f.write("".join(f"{s} : /nowhere/{s}.fasta\n" for s in ids))
    cf, md, fmt = (options_mode or mode).split(":")
    with open(os.path.join(root, "options.txt"), "w") as f:
        f.write(f"Options: dir={root}, verbosity=info, nb_threads=1, kmer_size={k}, minim_size=4, nb_parts={len(bodies)}, mode={md}, format={fmt}, count_format={cf}, until=all\n")
    P = len(bodies)
    table = (np.arange(256) % max(P, 1)).astype("<u2")
    with open(os.path.join(root, "repartition_gatb", "repartition.minimRepart"), "wb") as f:
        f.write(struct.pack("<HQH", P, len(table), 1)); f.write(table.tobytes()); f.write(struct.pack("<BI", 0, 0x12345678))
    with open(os.path.join(root, "hash.info"), "wb") as f:
        f.write(struct.pack("<QQQQI", window * P, P, window, 0, 4))
    ext = KINDS[mode][0]
    for p, body in enumerate(bodies):
        with open(os.path.join(root, "matrices", f"matrix_{p}.{ext}"), "wb") as f:
            f.write(matrix_header(mode, k, len(ids), p, window)); f.write(as_bytes(body))
    return root
