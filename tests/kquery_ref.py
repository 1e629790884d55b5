"""What `kmx query --kmer-index` (kmx_kquery_*) computes, restated from its definition with Python integers and one dictionary per
partition.

The index is one k-mer matrix per partition: rows in file order, keys strictly ascending as integers (word 0 the low 64 bits), a row
= ceil(k / 32) key words (low word first), then N u32 counts (COUNT) or ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3 (PA).
For a query sequence q and every position j whose k bases are all ACGT (either case):
  c = the canonical k-mer: min(forward, reverse complement) as integers with A0 C1 T2 G3, the first base the top digit
  p = repart[minimizer(c)]: the least m-mer value of its k - m + 1 m-mers (orc.minimizer_of: the split's table)
n_kmers[q] = the number of such positions; hits[q][i] = the number of them for which c is the key of a row of matrix p whose count i
is non-zero / whose bit i is set; sums[q][i] (COUNT) = that row's count i added up over the same positions.  Every occurrence counts.
A matrix of None is a partition that is not part of the call: its k-mers count in n_kmers and add nothing else."""
import struct
import numpy as np

import orc
from query_ref import _COMP, _value, random_reads, format_matrix, format_list, read_fasta_named      # noqa: F401 (the tests use them from here)

MODE_COUNT, MODE_PA = 0, 1


def stride_of(k, N, mode):
    return 8 * orc.kw_of_k(k) + (4 * N if mode == MODE_COUNT else (N + 7) // 8)


def kmer_place(kmer, k, m, lut, repart):
    """an upper-case ACGT k-mer -> (partition, the canonical k-mer as an integer)"""
    fwd = orc.kmer_from_string(kmer)
    rev = orc.kmer_from_string("".join(_COMP[c] for c in reversed(kmer)))
    c = fwd if _value(fwd) < _value(rev) else rev
    return int(repart[orc.minimizer_of(c, k, m, lut)]), _value(c)


def places(seqs, k, m, repart, lut=None):
    """per query the (partition, canonical k-mer) of every valid position, in position order -- the part of the restatement that does not
    depend on the index, so that tests over one set of reads work it out once"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    memo, out = {}, []
    for s in seqs:
        s = (s.decode() if isinstance(s, bytes) else s).upper()
        here = []
        for j in range(len(s) - k + 1):
            kmer = s[j:j + k]
            if any(ch not in _COMP for ch in kmer):
                continue
            if kmer not in memo:
                memo[kmer] = kmer_place(kmer, k, m, lut, repart)
            here.append(memo[kmer])
        out.append(here)
    return out


def tables_of(matrices, k, N, mode):
    """matrix bodies (uint8 arrays / bytes, or None) -> per partition a dictionary key -> row payload as an integer (little endian)"""
    kb, st = 8 * orc.kw_of_k(k), stride_of(k, N, mode)
    out = []
    for mt in matrices:
        if mt is None:
            out.append(None)
            continue
        raw = bytes(mt) if isinstance(mt, (bytes, bytearray, memoryview)) else np.ascontiguousarray(mt, np.uint8).tobytes()
        assert len(raw) % st == 0
        d, last = {}, -1
        for r in range(len(raw) // st):
            key = int.from_bytes(raw[r * st:r * st + kb], "little")
            assert key > last, "row keys must ascend strictly"
            last = key
            d[key] = int.from_bytes(raw[r * st + kb:(r + 1) * st], "little")
        out.append(d)
    return out


def kquery_expected(seqs, k, m, repart, N, mode, matrices, lut=None, at=None):
    """-> (n_kmers uint32[Q], hits uint32[Q, N], sums uint64[Q, N] -- zeros in PA mode); at: places(seqs, ...) when already known"""
    at = places(seqs, k, m, repart, lut) if at is None else at
    tabs = tables_of(matrices, k, N, mode)
    n_kmers, hits, sums = np.zeros(len(seqs), np.uint32), np.zeros((len(seqs), N), np.uint32), np.zeros((len(seqs), N), np.uint64)
    for q, here in enumerate(at):
        n_kmers[q] = len(here)
        h, s = {}, {}
        for p, key in here:
            if tabs[p] is None or key not in tabs[p]:
                continue
            row = tabs[p][key]
            if mode == MODE_PA:
                row &= (1 << N) - 1      # the padding bits dropped
                while row:
                    i = (row & -row).bit_length() - 1
                    h[i] = h.get(i, 0) + 1
                    row &= row - 1
            else:
                for i in range(N):
                    c = (row >> (32 * i)) & 0xFFFFFFFF
                    if c:
                        h[i] = h.get(i, 0) + 1
                        s[i] = s.get(i, 0) + c
        for i, c in h.items():
            hits[q, i] = c
        for i, c in s.items():
            sums[q, i] = c
    return n_kmers, hits, sums


def _sortable(keys2d):
    """uint64[n, kw] key words (low word first) -> an array np.searchsorted orders as the integers: uint64 for one word, Python integers else"""
    if keys2d.shape[1] == 1:
        return np.ascontiguousarray(keys2d[:, 0])
    out = np.empty(len(keys2d), dtype=object)
    for i, row in enumerate(keys2d):
        out[i] = _value(row)
    return out


def split_matrix(mt, k, N, mode):
    """a body -> (uint64[n, kw] keys, uint8[n, payload bytes])"""
    kb, st = 8 * orc.kw_of_k(k), stride_of(k, N, mode)
    a = (np.frombuffer(mt, np.uint8) if isinstance(mt, (bytes, bytearray, memoryview)) else np.ascontiguousarray(mt, np.uint8).reshape(-1)).reshape(-1, st)
    return np.ascontiguousarray(a[:, :kb]).view(np.uint64).reshape(len(a), kb // 8), a[:, kb:]


def kquery_expected_bulk(seqs, k, m, repart, N, mode, matrices, lut=None):
    """the same tables for inputs too long for the loop above, by another road: the CPU checker's split and k-mer count of one query at a
    time give, per partition, the distinct canonical k-mers with how often each occurs; np.searchsorted finds them among the matrix's
    keys; the rows found times those counts, summed.  tests/test_kquery_cpu.py holds the two against each other."""
    lut = orc.minimizer_lut(m) if lut is None else lut
    P = len(matrices)
    split = [None if mt is None else split_matrix(mt, k, N, mode) for mt in matrices]
    mkeys = [None if s is None else _sortable(s[0]) for s in split]
    n_kmers, hits, sums = np.zeros(len(seqs), np.uint32), np.zeros((len(seqs), N), np.uint64), np.zeros((len(seqs), N), np.uint64)
    for q, s in enumerate(seqs):
        s = (s.decode() if isinstance(s, bytes) else s).upper()
        if len(s) < k:
            continue
        for p, (recs, nk, _) in enumerate(orc.superk_partition([s], k, m, lut, repart, P)):
            if not nk:
                continue
            keys, cs = orc.count_kmer(recs, k, 1)
            n_kmers[q] += int(cs.sum(dtype=np.uint64))
            if mkeys[p] is None or not len(mkeys[p]):
                continue
            qk = _sortable(keys)
            at = np.minimum(np.searchsorted(mkeys[p], qk), len(mkeys[p]) - 1)
            found = mkeys[p][at] == qk
            found = found.astype(bool)
            rows, cnt = split[p][1][at[found]], cs[found].astype(np.uint64)
            if mode == MODE_PA:
                vals = np.unpackbits(rows, axis=1, bitorder="little")[:, :N].astype(np.uint64)
            else:
                vals = np.ascontiguousarray(rows).view(np.uint32).reshape(len(rows), N).astype(np.uint64)
            hits[q] += ((vals != 0).astype(np.uint64) * cnt[:, None]).sum(axis=0)
            if mode == MODE_COUNT:
                sums[q] += (vals * cnt[:, None]).sum(axis=0)
    return n_kmers, hits.astype(np.uint32), sums


def make_body(keys, payload, k):
    """ascending integer keys and uint8[n, payload bytes] -> the matrix body (uint8, one dimension)"""
    kw = orc.kw_of_k(k)
    if not len(keys):
        return np.zeros(0, np.uint8)
    kb = np.zeros((len(keys), 8 * kw), np.uint8)
    for r, key in enumerate(keys):
        kb[r] = np.frombuffer(int(key).to_bytes(8 * kw, "little"), np.uint8)
    return np.ascontiguousarray(np.concatenate([kb, np.ascontiguousarray(payload, np.uint8).reshape(len(keys), -1)], axis=1)).reshape(-1)


def read_keys(reads, k, m, repart, P, lut=None):
    """the distinct canonical k-mers of the reads per partition, ascending integers (the CPU checker's split and count)"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    out = []
    for recs, nk, _ in orc.superk_partition([r.upper() if isinstance(r, str) else r.upper() for r in reads if len(r) >= k], k, m, lut, repart, P):
        keys = orc.count_kmer(recs, k, 1)[0] if nk else np.zeros((0, orc.kw_of_k(k)), np.uint64)
        out.append([_value(row) for row in keys])
    return out


def synth_kindex(seed, N, P, k, m, mode, reads, frac, near=0.1, pad_ones=False, zeros=0.0, maxed=0.0, fill=0.5, keys=None):
    """a seeded index over the reads' own k-mers: every partition's matrix holds a fraction `frac` of the canonical k-mers the reads send
    there; for a share `near` of those the key is replaced by key - 1 or key + 1 as integers (a near miss: a comparison that ignores
    any one bit of any word finds what is not there).  COUNT rows: counts 1 .. 999, a share `zeros` of the cells 0 and a share `maxed`
    0xFFFFFFFF; PA rows: bits set with probability `fill`, the padding bits of the last byte all `pad_ones`.
    keys: read_keys(...) when already known.  -> (matrices: uint8 bodies, repart)"""
    rng = np.random.default_rng(seed)
    repart = orc.repart_static(m, P)
    keys = read_keys(reads, k, m, repart, P) if keys is None else keys
    top = 4 ** k
    mats = []
    for p in range(P):
        own = set(keys[p])
        kept = set()
        u = rng.random((len(keys[p]), 3))
        for i in np.nonzero(u[:, 0] < frac)[0]:
            key = keys[p][i]
            if u[i, 1] < near:
                miss = key + (1 if u[i, 2] < 0.5 else -1)
                if 0 <= miss < top and miss not in own:
                    key = miss
            kept.add(key)
        kept = sorted(kept)
        if mode == MODE_PA:
            bits = rng.random((len(kept), ((N + 7) // 8) * 8)) < fill
            bits[:, N:] = pad_ones
            payload = np.packbits(bits, axis=1, bitorder="little") if len(kept) else np.zeros((0, (N + 7) // 8), np.uint8)
        else:
            c = rng.integers(1, 1000, (len(kept), N)).astype(np.uint32)
            u = rng.random(c.shape)
            c[u < zeros] = 0
            c[u >= 1.0 - maxed] = 0xFFFFFFFF
            payload = c.view(np.uint8).reshape(len(kept), 4 * N)
        mats.append(make_body(kept, payload, k))
    return mats, repart


def format_sums(names, sample_ids, n_kmers, sums):
    """`kmx query --kmer-index --format sums`: the matrix layout with the u64 count sums in place of the hits"""
    return format_matrix(names, sample_ids, n_kmers, sums)


# ---- a run's matrix files (io/matrix_file.hpp: a 45-byte header, then the rows) -----------------------------------------------------
KM_MAGIC = 0x736b636972746d6b
MATRIX_MAGIC, PA_MAGIC = 0x6b5f78697274616d, 0x6b5f74616d6170


def read_matrix_file(path):
    """a plain (not lz4) .count / .pa file -> dict(k, n_cols, mode, body uint8)"""
    raw = open(path, "rb").read()
    magic, _, cpr, kind, k, slots = struct.unpack_from("<QIBQII", raw, 0)
    assert magic == KM_MAGIC and cpr == 0 and kind in (MATRIX_MAGIC, PA_MAGIC) and slots == orc.kw_of_k(k), path
    mode = MODE_COUNT if kind == MATRIX_MAGIC else MODE_PA
    n = struct.unpack_from("<I", raw, 33 if mode == MODE_COUNT else 29)[0]
    body = np.frombuffer(raw[45:], np.uint8)
    assert len(body) % stride_of(k, n, mode) == 0, path
    return dict(k=k, n_cols=n, mode=mode, body=body)
