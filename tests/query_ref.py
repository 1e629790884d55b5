"""What `kmx query` computes, restated from its definition with Python integers and a dictionary per query.

The index is a Bloom matrix per partition: W rows of ceil(N / 8) bytes, sample i = bit i & 7 of byte i >> 3.  For a query sequence q
and every position j whose k bases are all ACGT (either case):
  c   = the canonical k-mer: min(forward, reverse complement) as integers with A0 C1 T2 G3, the first base the top digit
  p   = repart[minimizer(c)]: the least m-mer value of its k - m + 1 m-mers (orc.minimizer_of: the split's table)
  h   = XXH64(c's ceil(k / 32) little-endian words, seed 0) % W
  row = matrix_p[h]
n_kmers[q] = the number of such positions; hits[q][i] = the number of them whose row has bit i set (i < N).  Every occurrence counts.
A matrix_p of None is a partition that is not part of the call: its k-mers count in n_kmers and add no hits."""
import numpy as np

import orc

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _value(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def kmer_address(kmer, k, m, lut, repart, W):
    """an upper-case ACGT k-mer -> (partition, row index)"""
    fwd = orc.kmer_from_string(kmer)
    rev = orc.kmer_from_string("".join(_COMP[c] for c in reversed(kmer)))
    c = fwd if _value(fwd) < _value(rev) else rev
    p = int(repart[orc.minimizer_of(c, k, m, lut)])
    return p, orc.xxh64(np.ascontiguousarray(c, np.uint64).tobytes()) % W


def query_expected(seqs, k, m, repart, W, N, matrices, lut=None):
    """seqs: strings; matrices[p]: uint8[W, ceil(N / 8)] or None -> (n_kmers uint32[Q], hits uint32[Q, N])"""
    lut = orc.minimizer_lut(m) if lut is None else lut
    n_kmers, hits = np.zeros(len(seqs), np.uint32), np.zeros((len(seqs), N), np.uint32)
    memo = {}
    for q, s in enumerate(seqs):
        s = (s.decode() if isinstance(s, bytes) else s).upper()
        per_col = {}
        n = 0
        for j in range(len(s) - k + 1):
            kmer = s[j:j + k]
            if any(ch not in _COMP for ch in kmer):
                continue
            n += 1
            if kmer not in memo:
                memo[kmer] = kmer_address(kmer, k, m, lut, repart, W)
            p, h = memo[kmer]
            if matrices[p] is None:
                continue
            row = int.from_bytes(matrices[p][h].tobytes(), "little") & ((1 << N) - 1)      # bit i = sample i; the padding bits dropped
            while row:
                i = (row & -row).bit_length() - 1
                per_col[i] = per_col.get(i, 0) + 1
                row &= row - 1
        n_kmers[q] = n
        for i, c in per_col.items():
            hits[q, i] = c
    return n_kmers, hits


def query_expected_bulk(seqs, k, m, repart, W, N, matrices, lut=None):
    """the same table for inputs too long for the loop above, by another road: the CPU checker's split and window-hash count of one
    query at a time give, per partition, the distinct row indices with how often each occurs; the rows' bits times those counts,
    summed.  tests/test_query_cpu.py holds the two against each other."""
    lut = orc.minimizer_lut(m) if lut is None else lut
    P = len(matrices)
    n_kmers, hits = np.zeros(len(seqs), np.uint32), np.zeros((len(seqs), N), np.uint64)
    for q, s in enumerate(seqs):
        s = (s.decode() if isinstance(s, bytes) else s).upper()
        if len(s) < k:
            continue
        for p, (recs, nk, _) in enumerate(orc.superk_partition([s], k, m, lut, repart, P)):
            if not nk:
                continue
            hs, cs = orc.count_hash(recs, k, W, p, 1)
            n_kmers[q] += int(cs.sum(dtype=np.uint64))
            if matrices[p] is None:
                continue
            bits = np.unpackbits(matrices[p][(hs - np.uint64(W * p)).astype(np.int64)], axis=1, bitorder="little")[:, :N]
            hits[q] += (bits.astype(np.uint64) * cs.astype(np.uint64)[:, None]).sum(axis=0)
    return n_kmers, hits.astype(np.uint32)


def synth_index(seed, N, W, P, k, m, fill, pad_ones=False):
    """a seeded index: P matrices uint8[W, ceil(N / 8)] whose bits are set with probability `fill`, and the static repartition table.
    pad_ones: every padding bit of every row's last byte is 1 (a result must never see them).  -> (matrices, repart)"""
    rng = np.random.default_rng(seed)
    nb = (N + 7) // 8
    mats = []
    for _ in range(P):
        bits = rng.random((W, nb * 8)) < fill
        bits[:, N:] = pad_ones
        mats.append(np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")))
    return mats, orc.repart_static(m, P)


def random_reads(seed, n, length, alphabet="ACGT"):
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alphabet.encode(), np.uint8)
    return [a[rng.integers(0, len(a), length)].tobytes().decode() for _ in range(n)]


def format_matrix(names, sample_ids, n_kmers, hits):
    """`kmx query --format matrix`: a header line, then one line per query with the integer hits"""
    out = ["\t".join(["query", "n_kmers"] + list(sample_ids))]
    for q, name in enumerate(names):
        out.append("\t".join([name, str(int(n_kmers[q]))] + [str(int(x)) for x in hits[q]]))
    return "\n".join(out) + "\n"


def format_list(names, sample_ids, n_kmers, hits, threshold=0.7):
    """`kmx query --format list`: query, sample, hits, n_kmers for every (query, sample) with n_kmers > 0 and hits >= T * n_kmers
    (compared as doubles), in query order, then column order"""
    out = []
    for q, name in enumerate(names):
        n = int(n_kmers[q])
        if n == 0:
            continue
        for i, sid in enumerate(sample_ids):
            if float(int(hits[q][i])) >= threshold * float(n):
                out.append(f"{name}\t{sid}\t{int(hits[q][i])}\t{n}\n")
    return "".join(out)


def read_fasta_named(path):
    """(first word of the header, sequence) per record of a plain FASTA file"""
    recs, name, seq = [], None, []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if name is not None:
                recs.append((name, "".join(seq)))
            name, seq = (line[1:].split() or [""])[0], []
        elif name is not None:
            seq.append(line)
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs
