"""The contract of kmx_kset_* and kmx_match_* (include/kmx.h, sections "kset" and "match") restated twice, with no code shared between the
two roads but the encoding, the list of cases the CPU and GPU tests share, and the keep rule and text formats of `kmx match`.

road A (match_strings): the header's own words -- Python strings and a dictionary, position by position.
road B (match_numpy):   numpy -- keys by a sliding window over the batch's digits, packed into byte strings whose order is the keys';
        the id of every position by searchsorted on the sorted distinct keys; everything else DERIVED FROM THE ID ARRAY: hits by
        add.reduceat, covered by a difference array, occ by bincount.

Encoding (the matrices' own): digit i (bits 2i, 2i + 1) of a key is base k - 1 - i, A0 C1 T2 G3; the complement is digit ^ 2."""
import functools
import random

import numpy as np

DIGIT = {"A": 0, "C": 1, "T": 2, "G": 3}
BASE = "ACTG"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NONE = 0xFFFFFFFF
HEADER = "read\tname\tlength\tkmers\thits\tfwd\tcovered\tfirst\tlast\n"


# ---- strings and integers -----------------------------------------------------------------------------------------------------------
def enc(s):
    v = 0
    for ch in s:
        v = v << 2 | DIGIT[ch]
    return v


def dec(v, k):
    return "".join(BASE[(v >> (2 * (k - 1 - j))) & 3] for j in range(k))


def rc_str(s):
    return "".join(COMP[c] for c in reversed(s))


def canon_of(s):
    """the canonical key of the k-mer s (upper case ACGT)"""
    return min(enc(s), enc(rc_str(s)))


def key_words_of(k):
    return (k + 31) // 32


def keys_to_words(keys, k):
    """list of integers -> uint64[n, key_words], low word first"""
    kw = key_words_of(k)
    a = np.zeros((len(keys), kw), np.uint64)
    for i, v in enumerate(keys):
        for w in range(kw):
            a[i, w] = (v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return a


class Match:
    """key_ids[n], n_distinct; recs: one (n_kmers, hits, fwd, covered, first, last) a read; ids: one per base of the batch; occ[n]"""

    def __init__(self, key_ids, recs, ids, occ):
        self.key_ids, self.recs, self.ids, self.occ = key_ids, recs, ids, occ
        self.n_distinct = sum(1 for v, j in enumerate(key_ids) if v == j)
        self.total_kmers, self.total_hits = sum(r[0] for r in recs), sum(r[1] for r in recs)

    def same(self, o):
        return self.key_ids == o.key_ids and self.recs == o.recs and self.ids == o.ids and self.occ == o.occ


# ---- road A ---------------------------------------------------------------------------------------------------------------------------
def match_strings(keys, k, reads):
    first_at = {}
    for v, x in enumerate(keys):
        first_at.setdefault(x, v)
    key_ids = [first_at[x] for x in keys]
    occ = [0] * len(keys)
    recs, ids = [], []
    for read in reads:
        up = read.upper()
        n_kmers = hits = fwd = 0
        covered = set()
        first = last = NONE
        row = [NONE] * len(read)
        for i in range(len(read) - k + 1):
            x = up[i:i + k]
            if any(ch not in DIGIT for ch in x):
                continue
            n_kmers += 1
            c = canon_of(x)
            if c not in first_at:
                continue
            j = first_at[c]
            hits += 1
            fwd += enc(x) == c
            covered.update(range(i, i + k))
            first = i if first == NONE else first
            last = i
            occ[j] += 1
            row[i] = j
        recs.append((n_kmers, hits, fwd, len(covered), first, last))
        ids += row
    return Match(key_ids, recs, ids, occ)


# ---- road B ---------------------------------------------------------------------------------------------------------------------------
_LUT = np.full(256, 4, np.uint8)
for _c, _d in DIGIT.items():
    _LUT[ord(_c)] = _LUT[ord(_c.lower())] = _d


def _pack(win):
    """rows of k digits, most significant first -> byte strings of ceil(k / 4) bytes whose order is the order of the keys"""
    m, k = win.shape
    nb = (k + 3) // 4
    pad = np.zeros((m, 4 * nb), np.uint8)
    pad[:, 4 * nb - k:] = win
    b = (pad[:, 0::4] << 6) | (pad[:, 1::4] << 4) | (pad[:, 2::4] << 2) | pad[:, 3::4]
    return np.ascontiguousarray(b).view(f"S{nb}").reshape(m) if m else np.zeros(0, f"S{nb}")


def match_numpy(keys, k, reads):
    n = len(keys)
    nb = (k + 3) // 4
    ks = np.array([int(x).to_bytes(nb, "big") for x in keys], f"S{nb}") if n else np.zeros(0, f"S{nb}")
    distinct, first_at = np.unique(ks, return_index=True)      # ascending; the index of the first occurrence: the least
    key_ids = first_at[np.searchsorted(distinct, ks)].tolist() if n else []
    lens = np.array([len(r) for r in reads], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    nbases = int(offs[-1])
    d = _LUT[np.frombuffer("".join(reads).encode(), np.uint8)] if nbases else np.zeros(0, np.uint8)
    ids = np.full(nbases, NONE, np.int64)
    valid = np.zeros(nbases, bool)
    strand = np.zeros(nbases, bool)
    if nbases >= k:
        m = nbases - k + 1
        win = np.lib.stride_tricks.sliding_window_view(d, k)
        bad = np.concatenate(([0], np.cumsum(d > 3)))
        ends = np.repeat(offs[1:], lens)[:m]
        ok = (bad[k:] - bad[:m] == 0) & (np.arange(m) + k <= ends)
        at = np.flatnonzero(ok)
        f, r = _pack(win[at]), _pack((win[at][:, ::-1] ^ 2) & 3)
        fw = f <= r
        c = np.where(fw, f, r)
        valid[at] = True
        if len(distinct) and len(at):
            where = np.minimum(np.searchsorted(distinct, c), len(distinct) - 1)
            found = distinct[where] == c
            ids[at[found]] = first_at[where[found]]
        strand[at] = fw
    hit = ids != NONE
    pos = np.arange(nbases)
    rel = pos - np.repeat(offs[:-1], lens)
    diff = np.zeros(nbases + k + 1, np.int64)
    np.add.at(diff, pos[hit], 1)
    np.add.at(diff, pos[hit] + k, -1)
    cov = np.cumsum(diff)[:nbases] > 0
    recs = [(0, 0, 0, 0, NONE, NONE)] * len(reads)
    full = np.flatnonzero(lens > 0)
    if len(full):
        seg = offs[full]

        def per_read(a):
            return np.add.reduceat(a.astype(np.int64), seg)
        nk, nh, nf, nc = per_read(valid), per_read(hit), per_read(hit & strand), per_read(cov)
        lo = np.minimum.reduceat(np.where(hit, rel, 1 << 40), seg)
        hi = np.maximum.reduceat(np.where(hit, rel, -1), seg)
        for i, q in enumerate(full.tolist()):
            recs[q] = (int(nk[i]), int(nh[i]), int(nf[i]), int(nc[i]), int(lo[i]) if nh[i] else NONE, int(hi[i]) if nh[i] else NONE)
    occ = np.bincount(ids[hit], minlength=n).tolist() if n else []
    return Match(key_ids, recs, ids.tolist(), occ)


# ---- the header's worked example --------------------------------------------------------------------------------------------------
EXAMPLE = dict(k=5, strs=("TTGCA", "ATTGC", "TTGCA", "TGCAC"), keys=(692, 173, 692, 721), key_ids=[0, 1, 0, 3], n_distinct=3,
               reads=("CATTGCAC", "ttgcaNtgcaat", "ACGT", "GGGGGGG", "TGCAC"),
               recs=[(4, 3, 3, 7, 1, 3), (3, 3, 1, 11, 0, 7), (0, 0, 0, 0, NONE, NONE), (3, 0, 0, 0, NONE, NONE), (1, 1, 1, 5, 0, 0)],
               occ=[3, 2, 0, 2], ids={1: 1, 2: 0, 3: 3, 8: 0, 14: 0, 15: 1, 31: 3})


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
K_SWEEP = (8, 12, 31, 32, 33, 63, 64, 65, 96, 97, 126, 127)
TILE_LENS = ("k-1", "k", "k+1", 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
COVER_POS = (0, 63, 64, 127, 128)
SET_N = (0, 1, 2, 255, 256, 257, 4097)
PAL_K = (8, 32, 64, 96, 126)      # an even k of every key_words class (1, 1, 2, 3, 4)
POLY_HITS = 100000


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def kmers_of(reads, k):
    """the canonical key of every valid position of every read, in order, duplicates and all"""
    out = []
    for r in reads:
        up = r.upper()
        for i in range(len(r) - k + 1):
            x = up[i:i + k]
            if all(ch in DIGIT for ch in x):
                out.append(canon_of(x))
    return out


def distinct(keys):
    return list(dict.fromkeys(keys))


def flipped(key, k, w, own, rng):
    """key with one bit of word w flipped, still canonical and no k-mer of `own`; None when word w holds none of the 2 k bits"""
    bits = [b for b in range(64 * w, min(64 * w + 64, 2 * k))]
    rng.shuffle(bits)
    for b in bits:
        y = key ^ (1 << b)
        if y == canon_of(dec(y, k)) and y not in own:
            return y
    return None


def unique_hit_read(rng, k, length, places):
    """a random read in which the k-mers at `places` occur (on either strand) nowhere else"""
    while True:
        r = rand_seq(rng, length)
        ks = kmers_of([r], k)
        if all(ks.count(ks[p]) == 1 for p in places):
            return r, [ks[p] for p in places]


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, k, keys, reads)]: keys a list of canonical integers (duplicates where the case is about them), reads a list of strings"""
    out = []
    # key_words and the top-word mask: the set is the reads' own k-mers, a share replaced by the key with one bit flipped in each word in turn
    for k in K_SWEEP:
        rng = random.Random(1000 + k)
        reads = [rand_seq(rng, k + 40), rand_seq(rng, k + 7).lower(), rand_seq(rng, 2 * k + 3)]
        keys = distinct(kmers_of(reads, k))
        own = set(keys)
        for i in range(0, len(keys), 3):
            y = flipped(keys[i], k, (i // 3) % key_words_of(k), own, rng)
            if y is not None:
                keys[i] = y
        rng.shuffle(keys)
        out.append((f"words_k{k}", k, keys, reads))
    # tiles: every length on either side of a tile's edge, empty reads between them, N at the first and the last base of a k-mer, lower case
    for k in (8, 31):
        rng = random.Random(2000 + k)
        reads = []
        for L in TILE_LENS:
            L = {"k-1": k - 1, "k": k, "k+1": k + 1}.get(L, L)
            reads += [rand_seq(rng, L), ""]
        r = list(rand_seq(rng, 4 * k + 10))
        r[k] = "N"; r[3 * k] = "n"      # the k-mer at 1 ends on it, the one at k starts with it; so for 2 k + 1 and 3 k
        reads += ["".join(r), "", "", rand_seq(rng, 70).lower(), rand_seq(rng, 2 * k + 1)]
        keys = distinct(kmers_of(reads, k))[::2]
        out.append((f"tiles_k{k}", k, keys, reads))
    # read boundaries at lanes 0, 1 and 63 of a tile; the last read ends inside a tile
    rng = random.Random(2100)
    reads = [rand_seq(rng, L) for L in (64, 65, 62, 40)]
    out.append(("bounds_k8", 8, distinct(kmers_of(reads, 8))[1::2], reads))
    out.append(("no_reads", 31, distinct(kmers_of([rand_seq(rng, 80)], 31)), []))
    out.append(("empty_reads_only", 31, distinct(kmers_of([rand_seq(rng, 80)], 31)), ["", "", ""]))
    rng = random.Random(2200)
    long = rand_seq(rng, 200000)
    reads = [rand_seq(rng, 50), "", rand_seq(rng, 33), long, rand_seq(rng, 90)]
    out.append(("long_read_k31", 31, distinct(kmers_of([long[i:i + 31] for i in range(0, 199000, 50)] + reads[:1], 31)), reads))
    rng = random.Random(2300)
    reads = [rand_seq(rng, 30) for _ in range(5000)]
    out.append(("many_reads_k12", 12, distinct(kmers_of(reads[:100], 12)), reads))
    # cover: one hit at a position on either side of a tile's edge, at the shortest and the longest k (126 bases back: two tiles)
    for k in (8, 127):
        for p in COVER_POS:
            rng = random.Random(3000 + 10 * k + p)
            r, ks = unique_hit_read(rng, k, p + k + 70, [p])
            out.append((f"cover_k{k}_p{p}", k, ks, [r, rand_seq(rng, 20)]))
        for d in (k - 1, k, k + 1):      # two hits: one shared base, none and abutting, one base between them
            rng = random.Random(3500 + 10 * k + d)
            r, ks = unique_hit_read(rng, k, 60 + 2 * k + 70, [60, 60 + d])
            out.append((f"cover_k{k}_gap{d - k}", k, ks, [rand_seq(rng, 9), r]))
        rng = random.Random(3600 + k)
        reads = [rand_seq(rng, 300), rand_seq(rng, k), rand_seq(rng, k + 64)]
        out.append((f"cover_k{k}_all", k, distinct(kmers_of(reads, k)), reads))
    # a hit that ends on its read's last base, the next read starting in the same tile: nothing leaks
    for k in (8, 31):
        rng = random.Random(3700 + k)
        a, ks = unique_hit_read(rng, k, 40, [40 - k])
        while True:
            b = rand_seq(rng, 100)
            if not set(kmers_of([b, a[-(k - 1):] + b[:k - 1]], k)) & set(ks):
                break
        out.append((f"cover_k{k}_last_base", k, ks, [a, b]))
    # the set: sizes on either side of a workgroup, duplicates, palindromes
    rng = random.Random(4000)
    pool_read = rand_seq(rng, 6000)
    pool = distinct(kmers_of([pool_read], 31))
    for n in SET_N:
        out.append((f"set_n{n}", 31, pool[:n], [pool_read[:300], rand_seq(rng, 100), pool_read[4000:4200]]))
    rng = random.Random(4100)
    src = rand_seq(rng, 400)
    base = distinct(kmers_of([src], 31))[:60]
    keys = [x for i, x in enumerate(base) for _ in range(1 + (i * 7) % 50)]
    rng.shuffle(keys)
    out.append(("dups_k31", 31, keys, [src, rc_str(src[:200]), rand_seq(rng, 64)]))
    rng = random.Random(4200)
    src = rand_seq(rng, 330)
    for k in (31, 64):
        out.append((f"n300_k{k}", k, distinct(kmers_of([src], k))[:300][::-1] if k == 31 else distinct(kmers_of([src + rand_seq(rng, 40)], k))[:300],
                    [src, rand_seq(rng, 100)]))
    for k in PAL_K:
        rng = random.Random(4300 + k)
        half = rand_seq(rng, k // 2)
        pal = half + rc_str(half)
        reads = [rand_seq(rng, 10) + pal + rand_seq(rng, 10), pal.lower(), rand_seq(rng, k + 5)]
        keys = [enc(pal)] + distinct(kmers_of(reads[2:], k))[:3]
        out.append((f"palindrome_k{k}", k, keys, reads))
    # occ under contention: one key hit 10^5 times on each strand
    out.append(("poly_a_k31", 31, [enc("A" * 31), enc("A" * 30 + "C")], ["A" * (POLY_HITS + 30), "ACGT", "T" * 500]))
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """road A on the named case, computed once"""
    _, k, keys, reads = case(name)
    return match_strings(keys, k, reads)


# ---- `kmx match`: the keep rule and the text formats ---------------------------------------------------------------------------------
def kept(rec, length, min_hits=1, min_frac=None, min_cover=None, invert=False):
    n_kmers, hits, _, covered = rec[:4]
    keep = hits >= min_hits
    if min_frac is not None:
        keep = keep and float(hits) >= min_frac * float(n_kmers)
    if min_cover is not None:
        keep = keep and float(covered) >= min_cover * float(length)
    if min_frac is not None or min_cover is not None:
        keep = keep and n_kmers > 0
    return keep != invert


def name_of(header):
    """the first word of a header line behind its '>' / '@'"""
    for i, ch in enumerate(header):
        if ch in " \t\r":
            return header[1:i]
    return header[1:]


def output_text(headers, reads, recs):
    def dash(x):
        return "-" if x == NONE else str(x)
    return HEADER + "".join(f"{q}\t{name_of(h)}\t{len(s)}\t{r[0]}\t{r[1]}\t{r[2]}\t{r[3]}\t{dash(r[4])}\t{dash(r[5])}\n"
                            for q, (h, s, r) in enumerate(zip(headers, reads, recs)))


def extract_text(headers, reads, quals, recs, **rule):
    """quals[q] None: a FASTA record, a header and one sequence line; else four lines"""
    out = []
    for h, s, ql, r in zip(headers, reads, quals, recs):
        if kept(r, len(s), **rule):
            h2 = f"{h} KM:i:{r[0]} HT:i:{r[1]} FW:i:{r[2]} CV:i:{r[3]}"
            out.append(f"{h2}\n{s}\n" if ql is None else f"{h2}\n{s}\n+\n{ql}\n")
    return "".join(out)


def kmer_counts_text(keys, k, key_ids, occ):
    return "kmer\tcount\n" + "".join(f"{dec(keys[v], k)}\t{occ[v]}\n" for v in range(len(keys)) if key_ids[v] == v)


def positions_text(k, reads, ids):
    """read, position in it, the key's id, + when the read shows the key itself"""
    out, at = ["read\tpos\tkmer_index\tstrand\n"], 0
    for q, s in enumerate(reads):
        for i in range(len(s)):
            if ids[at + i] != NONE:
                x = s[i:i + k].upper()
                out.append(f"{q}\t{i}\t{ids[at + i]}\t{'+' if enc(x) == canon_of(x) else '-'}\n")
        at += len(s)
    return "".join(out)


def parse_kmers(text):
    """`--kmers`: the first tab-separated field of every line that is not empty, does not start with # and is not the header `kmer ...`;
    k is the first k-mer's length -> (k, the canonical keys in file order, duplicates kept); ValueError with the line otherwise"""
    k, out = None, []
    for ln, line in enumerate(text.split("\n"), 1):
        line = line.rstrip("\r")
        if not line or line[0] == "#":
            continue
        s = line.split("\t")[0]
        if s == "kmer":
            continue
        k = len(s) if k is None else k
        if len(s) != k:
            raise ValueError(f"line {ln}: a k-mer of {len(s)} characters, the first has {k}")
        if any(c not in "ACGTacgt" for c in s):
            raise ValueError(f"line {ln}: malformed k-mer")
        out.append(canon_of(s.upper()))
    return k, out


def parse_records(text):
    """FASTA / FASTQ text -> [(header line, sequence, quality or None)]: sequence lines joined, blanks and carriage returns dropped"""
    recs, lines, i = [], text.split("\n"), 0
    while i < len(lines):
        line = lines[i].rstrip("\r")
        if line[:1] == ">":
            seq, i = [], i + 1
            while i < len(lines) and lines[i][:1] != ">":
                seq.append(lines[i])
                i += 1
            recs.append((line, "".join("".join(seq).split()), None))
        elif line[:1] == "@":
            seq, i = [], i + 1
            while i < len(lines) and lines[i][:1] != "+":
                seq.append(lines[i])
                i += 1
            s, q, i = "".join("".join(seq).split()), "", i + 1
            while i < len(lines) and len(q) < len(s):
                q += lines[i].rstrip("\r")
                i += 1
            recs.append((line, s, q))
        else:
            i += 1
    return recs
