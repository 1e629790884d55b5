"""What `kmx query` computes over a counting Bloom index (a `--mode hash:bfc:bin` run), restated from its definition (include/kmx.h,
section "cquery") by two roads that share no code beyond the k-mer's address.

The index is a matrix per partition: W rows of nb = ceil(N * w / 8) bytes.  Bit position t of a row is bit 7 - (t & 7) of byte t >> 3;
sample i's class v_i is the w bits at positions i * w ... i * w + w - 1, the first the most significant.  For a query q and every
position whose k bases are all ACGT (either case), with (p, h) the k-mer's address as tests/query_ref.py has it:
  n_kmers[q]   the number of such positions
  hits[q][i]   the number of them whose v_i >= min_class
  sums[q][i]   the sum of floor_of(v_i) over them; floor_of(0) = 0, floor_of(v) = 2^(min(v, 32) - 1)
A matrix_p of None is a partition that is not part of the call: its k-mers count in n_kmers and add nothing else."""
import numpy as np

import orc
import query_ref as qr


def floor_of(v):
    """the smallest count the merge maps to class v (a lower bound for the top class); classes above 32 stand in no merged body"""
    return 0 if v == 0 else 1 << (min(v, 32) - 1)


def cquery_expected(seqs, k, m, repart, W, N, matrices, w, min_class=1, lut=None):
    """road 1: Python integers and one dictionary per query.  matrices[p]: uint8[W, nb] or None
    -> (n_kmers uint32[Q], hits uint32[Q, N], sums uint64[Q, N])"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    nb = (N * w + 7) // 8
    n_kmers, hits, sums = np.zeros(len(seqs), np.uint32), np.zeros((len(seqs), N), np.uint32), np.zeros((len(seqs), N), np.uint64)
    memo = {}
    for q, s in enumerate(seqs):
        s = (s.decode() if isinstance(s, bytes) else s).upper()
        per_col = {}
        n = 0
        for j in range(len(s) - k + 1):
            kmer = s[j:j + k]
            if any(ch not in "ACGT" for ch in kmer):
                continue
            n += 1
            if kmer not in memo:
                memo[kmer] = qr.kmer_address(kmer, k, m, lut, repart, W)
            p, h = memo[kmer]
            if matrices[p] is None:
                continue
            row = np.asarray(matrices[p]).reshape(W, nb)[h].tobytes()
            R = int.from_bytes(row, "big")
            for i in range(N):
                v = (R >> (8 * nb - (i + 1) * w)) & ((1 << w) - 1)
                if v:
                    hc, sc = per_col.get(i, (0, 0))
                    per_col[i] = (hc + (v >= min_class), sc + floor_of(v))
        n_kmers[q] = n
        for i, (hc, sc) in per_col.items():
            hits[q, i], sums[q, i] = hc, sc
    return n_kmers, hits, sums


def unpack_classes(rows, N, w):
    """uint8[n, nb] -> uint32[n, N]: the classes of every row (numpy, unpackbits in MSB-first order)"""
    rows = np.asarray(rows, np.uint8)
    bits = np.unpackbits(rows, axis=1, bitorder="big")[:, :N * w].reshape(len(rows), N, w).astype(np.uint32)
    return (bits << np.arange(w - 1, -1, -1, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)


def np_addresses(seqs, k, m, repart, W, P, lut=None):
    """per query, per partition that holds any of its k-mers: (p, row indices int64[n], occurrences uint64[n]) from the CPU checker's
    split and window-hash count of one query at a time (as query_ref.query_expected_bulk)"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    out = []
    for s in seqs:
        s = (s.decode() if isinstance(s, bytes) else s).upper()
        mine = []
        if len(s) >= k:
            for p, (recs, nk, _) in enumerate(orc.superk_partition([s], k, m, lut, repart, P)):
                if nk:
                    hs, cs = orc.count_hash(recs, k, W, p, 1)
                    mine.append((p, (hs - np.uint64(W * p)).astype(np.int64), cs.astype(np.uint64)))
        out.append(mine)
    return out


def np_expected_at(addresses, W, N, matrices, w, min_class=1):
    """the tables from np_addresses' output: the rows' classes by numpy"""
    nb = (N * w + 7) // 8
    Q = len(addresses)
    n_kmers, hits, sums = np.zeros(Q, np.uint32), np.zeros((Q, N), np.uint64), np.zeros((Q, N), np.uint64)
    for q, mine in enumerate(addresses):
        for p, hs, cs in mine:
            n_kmers[q] += int(cs.sum(dtype=np.uint64))
            if matrices[p] is None:
                continue
            v = unpack_classes(np.asarray(matrices[p]).reshape(W, nb)[hs], N, w)
            shift = np.maximum(np.minimum(v, 32), 1).astype(np.uint64) - np.uint64(1)
            fl = np.where(v == 0, np.uint64(0), np.uint64(1) << shift)
            hits[q] += ((v >= min_class).astype(np.uint64) * cs[:, None]).sum(axis=0, dtype=np.uint64)
            sums[q] += (fl * cs[:, None]).sum(axis=0, dtype=np.uint64)
    return n_kmers, hits.astype(np.uint32), sums


def cquery_expected_np(seqs, k, m, repart, W, N, matrices, w, min_class=1, lut=None):
    """road 2: numpy with unpackbits(bitorder="big"); the addresses come from orc.superk_partition and orc.count_hash"""
    return np_expected_at(np_addresses(seqs, k, m, repart, W, len(matrices), lut), W, N, matrices, w, min_class)


def pack_classes(classes, w, pad_ones=False):
    """uint[W, N] classes below 2^w -> uint8[W, ceil(N * w / 8)]: field i at bit positions i * w ..., MSB first; pad_ones: every
    padding bit behind position N * w is 1 (a result must never see them)"""
    classes = np.asarray(classes, np.uint32)
    W, N = classes.shape
    assert int(classes.max(initial=0)) < (1 << w)
    nb = (N * w + 7) // 8
    bits = np.zeros((W, nb * 8), np.uint8)
    bits[:, :N * w] = ((classes[:, :, None] >> np.arange(w - 1, -1, -1, dtype=np.uint32)) & 1).reshape(W, N * w)
    bits[:, N * w:] = 1 if pad_ones else 0
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="big"))


def synth_index_bfc(seed, N, W, P, k, m, w, pad_ones=False, dist="uniform"):
    """a seeded counting index: P matrices uint8[W, ceil(N * w / 8)] and the static repartition table.  dist: "uniform" (classes
    0 ... 2^w - 1 alike), "zero" (an all-zero body), "ones" (every bit of the body set, padding included), or an integer (every
    class is that one).  -> (matrices, repart)"""
    rng = np.random.default_rng(seed)
    nb = (N * w + 7) // 8
    mats = []
    for _ in range(P):
        if dist == "ones":
            mats.append(np.full((W, nb), 0xFF, np.uint8))
            continue
        if dist == "uniform":      # (every class alike is every bit a coin: random bytes, then the padding bits)
            mt = rng.integers(0, 256, (W, nb), dtype=np.uint8)
            pad = np.uint8(0xFF >> ((N * w) % 8)) if (N * w) % 8 else np.uint8(0)
            mt[:, -1] = (mt[:, -1] | pad) if pad_ones else (mt[:, -1] & ~pad)
            mats.append(mt)
            continue
        if dist == "zero":
            cl = np.zeros((W, N), np.uint32)
        else:
            cl = np.full((W, N), int(dist), np.uint32)
        mats.append(pack_classes(cl, w, pad_ones))
    return mats, orc.repart_static(m, P)


def format_sums(names, sample_ids, n_kmers, sums):
    """`kmx query --format sums`: the matrix layout with the u64 sums in place of the hits"""
    return qr.format_matrix(names, sample_ids, n_kmers, sums)
