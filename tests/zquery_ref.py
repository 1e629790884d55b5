"""What `kmx query --z` computes, restated from its definition by two roads.

Everything of query_ref.py stands: the index, what a valid position is, the canonical k-mer, the partition, the row, the padding
bits.  Let K = k + z.  Position j of a query is a K-position when j + K <= the query's end and all K bases from j on are ACGT (either
case).  n_kmers[q] = the K-positions of q; hits[q][i] = the K-positions j for which bit i is set in the row of EVERY k-mer at j, j + 1,
..., j + z.  A k-mer of a partition whose matrix is None has a row of zeros: its windows count in n_kmers and add no hit.

  zquery_expected      Python integers: a row integer per valid position (query_ref.kmer_address), then the AND over each window
  zquery_expected_np   numpy: the addresses of all positions at once (the canonical k-mer, XXH64 and the window minimum of the m-mer
                       values worked out on arrays, nothing shared with the road above but the minimizer table), an unpacked
                       positions x N boolean matrix, a sliding logical_and, sums per query
tests/test_zquery_cpu.py holds the two against each other."""
import numpy as np

import orc
import query_ref as qr

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _text(s):
    return s.decode() if isinstance(s, bytes) else s


def zquery_expected(seqs, k, z, m, repart, W, N, matrices, lut=None):
    """seqs: strings; matrices[p]: uint8[W, ceil(N / 8)] or None -> (n_kmers uint32[Q], hits uint32[Q, N])"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    K = k + z
    n_kmers, hits = np.zeros(len(seqs), np.uint32), np.zeros((len(seqs), N), np.uint32)
    memo = {}
    for q, s in enumerate(seqs):
        s = _text(s).upper()
        rows = []      # per position: None (no valid k-mer) or the row's bits below N as an integer
        for j in range(len(s) - k + 1):
            kmer = s[j:j + k]
            if any(ch not in _COMP for ch in kmer):
                rows.append(None)
                continue
            if kmer not in memo:
                memo[kmer] = qr.kmer_address(kmer, k, m, lut, repart, W)
            p, h = memo[kmer]
            rows.append(0 if matrices[p] is None else int.from_bytes(matrices[p][h].tobytes(), "little") & ((1 << N) - 1))
        n = 0
        for j in range(len(s) - K + 1):
            if any(ch not in _COMP for ch in s[j:j + K]):
                continue
            n += 1
            a = (1 << N) - 1
            for t in range(z + 1):
                a &= rows[j + t]      # (a K-position: none of them is None)
            while a:
                hits[q, (a & -a).bit_length() - 1] += 1
                a &= a - 1
        n_kmers[q] = n
    return n_kmers, hits


# ---- the numpy road ------------------------------------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = (np.uint64(x) for x in (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5))


def _rotl(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _round(acc, w):
    return _rotl(acc + w * _P2, 31) * _P1


def xxh64_words(words):
    """XXH64, seed 0, of len(words) little-endian u64 words (1 .. 4) per element: words a list of uint64 arrays"""
    n = 8 * len(words)
    with np.errstate(over="ignore"):
        if len(words) == 4:      # 32 bytes: one stripe through the four accumulators
            v = [_round(s, w) for s, w in zip((_P1 + _P2, _P2, np.uint64(0), np.uint64(0) - _P1), words)]
            h = _rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)
            for x in v:
                h = (h ^ _round(np.uint64(0), x)) * _P1 + _P4
            h = h + np.uint64(n)
        else:
            h = np.full(len(words[0]), _P5 + np.uint64(n), np.uint64)
            for w in words:
                h = _rotl(h ^ _round(np.uint64(0), w), 27) * _P1 + _P4
        h = h ^ (h >> np.uint64(33)); h = h * _P2; h = h ^ (h >> np.uint64(29)); h = h * _P3; h = h ^ (h >> np.uint64(32))
    return h


_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate("ACTG"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def addresses_np(seqs, k, m, repart, W, lut=None):
    """the concatenated queries position by position -> dict(starts, lens, ok bool[L]: a valid k-mer of its query starts here,
    part int64[L], row int64[L] (both meaningless where not ok), bad int64[L + 1]: non-ACGT bases in front of each position)"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    blob = "".join(_text(s) for s in seqs).encode()
    lens = np.array([len(s) for s in seqs], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    L = len(blob)
    raw = _CODE[np.frombuffer(blob, np.uint8)] if L else np.zeros(0, np.uint8)
    bad = np.concatenate([[0], np.cumsum(raw == 255)]).astype(np.int64)
    out = dict(starts=starts, lens=lens, bad=bad, ok=np.zeros(L, bool), part=np.zeros(L, np.int64), row=np.zeros(L, np.int64))
    n = L - k + 1
    if n <= 0:
        return out
    codes = (raw & 3).astype(np.uint64)
    kw = (k + 31) // 32
    fwd, rev = [np.zeros(n, np.uint64) for _ in range(kw)], [np.zeros(n, np.uint64) for _ in range(kw)]
    for d in range(k):      # digit d of the forward k-mer is base k - 1 - d, of the reverse complement base d complemented (^ 2)
        sh = np.uint64(2 * (d % 32))
        fwd[d // 32] |= codes[k - 1 - d:k - 1 - d + n] << sh
        rev[d // 32] |= (codes[d:d + n] ^ np.uint64(2)) << sh
    less, decided = np.zeros(n, bool), np.zeros(n, bool)
    for w in range(kw - 1, -1, -1):      # the most significant word first
        ne = ~decided & (fwd[w] != rev[w])
        less |= ne & (fwd[w] < rev[w])
        decided |= ne
    canon = [np.where(less, f, r) for f, r in zip(fwd, rev)]
    row = (xxh64_words(canon) % np.uint64(W)).astype(np.int64)
    nm = L - m + 1
    mm = np.zeros(nm, np.uint64)
    for i in range(m):      # an m-mer's first base is its top digit
        mm = (mm << np.uint64(2)) | codes[i:i + nm]
    val = lut[mm.astype(np.int64)]
    mini = val[:n].copy()
    for i in range(1, k - m + 1):
        np.minimum(mini, val[i:i + n], out=mini)
    pos = np.arange(n, dtype=np.int64)
    end = np.repeat(starts[1:], lens)[:n]      # the end of the query that holds the position
    out["ok"][:n] = (bad[k:k + n] == bad[:n]) & (pos + k <= end)
    out["part"][:n] = np.asarray(repart)[mini.astype(np.int64)].astype(np.int64)
    out["row"][:n] = row
    return out


def windows_np(A, rowbytes, k, z, N):
    """A: addresses_np's output; rowbytes uint8[L, ceil(N / 8)]: the matrix row of every position's k-mer, zeros where there is none
    (or its partition is in no call) -> (n_kmers, hits): a sliding logical_and over the unpacked rows, sums per query"""
    starts, lens, bad = A["starts"], A["lens"], A["bad"]
    L, K, Q = len(A["ok"]), k + z, len(lens)
    n_kmers, hits = np.zeros(Q, np.uint32), np.zeros((Q, N), np.uint32)
    n = L - K + 1
    if n <= 0:
        return n_kmers, hits
    B = np.unpackbits(rowbytes, axis=1, bitorder="little")[:, :N].astype(bool)      # positions x N; the padding bits dropped
    acc = B[:n].copy()
    for t in range(1, z + 1):
        np.logical_and(acc, B[t:t + n], out=acc)
    end = np.repeat(starts[1:], lens)[:n]
    kpos = (bad[K:K + n] == bad[:n]) & (np.arange(n, dtype=np.int64) + K <= end)      # K bases of ACGT that end inside the query
    acc &= kpos[:, None]
    for q in range(Q):
        s, e = int(starts[q]), min(int(starts[q + 1]), n)
        if e > s:
            n_kmers[q] = int(kpos[s:e].sum())
            hits[q] = acc[s:e].sum(axis=0, dtype=np.uint32)
    return n_kmers, hits


def zquery_expected_np(seqs, k, z, m, repart, W, N, matrices, lut=None, addr=None):
    """the same tables by the numpy road; addr: addresses_np's output for the same (seqs, k, m, repart, W), when at hand"""
    A = addresses_np(seqs, k, m, repart, W, lut) if addr is None else addr
    rowbytes = np.zeros((len(A["ok"]), (N + 7) // 8), np.uint8)
    for p, mt in enumerate(matrices):
        if mt is None:
            continue
        sel = np.nonzero(A["ok"] & (A["part"] == p))[0]
        if len(sel):
            rowbytes[sel] = np.asarray(mt)[A["row"][sel]]
    return windows_np(A, rowbytes, k, z, N)
