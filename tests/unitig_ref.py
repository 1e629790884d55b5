"""The contract of kmx_unitigs_* and kmx_groupsum_* (include/kmx.h, sections "unitigs" and "groupsum") restated twice, with no code shared
between the two roads, the list of cases the CPU and GPU tests share, and kmx_groupsum_* in numpy and in plain loops.

road A (unitigs_links): the header's own words -- extensions, degrees, candidates and mutual links over a dictionary of Python integers,
        then every component of the link graph walked from its ends.
road B (unitigs_walk):  a walker over strings: from a k-mer, extend while the successor is unique both ways.

Encoding (the matrices' own): digit i (bits 2i, 2i + 1) of a key is base k - 1 - i, A0 C1 T2 G3; the complement is digit ^ 2."""
import random

import numpy as np

DIGIT = {"A": 0, "C": 1, "T": 2, "G": 3}
BASE = "ACTG"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NONE = None


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


def rc_int(v, k):
    r = 0
    for _ in range(k):
        r = r << 2 | ((v & 3) ^ 2)
        v >>= 2
    return r


def canon_int(v, k):
    return min(v, rc_int(v, k))


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


class Unitigs:
    """what a call gives: U, unitig / pos / ori per node, start / len / circ per unitig, seqs a list of strings"""

    def __init__(self, unitig, pos, ori, start, length, circ, seqs):
        self.U = len(start)
        self.unitig, self.pos, self.ori, self.start, self.len, self.circ, self.seqs = unitig, pos, ori, start, length, circ, seqs

    def seq_off(self, k):
        off = [0]
        for n in self.len:
            off.append(off[-1] + n + k - 1)
        return off

    def same(self, o):
        return (self.U == o.U and self.unitig == o.unitig and self.pos == o.pos and self.ori == o.ori and self.start == o.start and
                self.len == o.len and self.circ == o.circ and self.seqs == o.seqs)


# ---- road A: links over a dictionary of integers ----------------------------------------------------------------------------------
def extensions(keys, index, k, v, s):
    """the present extensions of side s of node v, as (u, t, y) in the order of c"""
    mask = (1 << (2 * k)) - 1
    x = keys[v]
    out = []
    for c in range(4):
        y = ((x << 2) & mask) | c if s == 1 else (x >> 2) | (c << (2 * (k - 1)))
        u = index.get(canon_int(y, k))
        if u is None:
            continue
        if s == 1:
            t = 0 if y == keys[u] else 1
        else:
            t = 1 if y == keys[u] else 0
        out.append((u, t, y))
    return out


def links_of(keys, k):
    """-> (link, deg): link[2v + s] = 2u + t or None; deg[2v + s]"""
    n = len(keys)
    index = {x: i for i, x in enumerate(keys)}
    pal = [x == rc_int(x, k) for x in keys]
    cand, deg = [None] * (2 * n), [0] * (2 * n)
    for v in range(n):
        for s in (0, 1):
            e = extensions(keys, index, k, v, s)
            deg[2 * v + s] = len(e)
            if len(e) == 1:
                u, t, _ = e[0]
                if u != v and not pal[v] and not pal[u]:
                    cand[2 * v + s] = 2 * u + t
    link = [c if c is not None and cand[c] == a else None for a, c in enumerate(cand)]
    return link, deg


def _oriented(keys, k, v, o):
    return keys[v] if o == 0 else rc_int(keys[v], k)


def unitigs_links(keys, k):
    n = len(keys)
    link, _ = links_of(keys, k)
    unitig_start, pos, ori = [None] * n, [None] * n, [None] * n
    length, circ = {}, {}

    def lay(a, count, start, is_circ):      # `count` nodes from state a (node a >> 1 left through side a & 1)
        for i in range(count):
            w, r = a >> 1, a & 1
            unitig_start[w], pos[w], ori[w] = start, i, r ^ 1
            if i + 1 < count:
                a = link[a] ^ 1
        length[start], circ[start] = count, is_circ

    for v in range(n):
        if unitig_start[v] is not None:
            continue
        # travel from v through side 1 until the path ends or v comes round again
        a, seen, cyc = 2 * v + 1, [2 * v + 1], False
        while link[a] is not None:
            a = link[a] ^ 1
            if a == 2 * v + 1:
                cyc = True
                break
            seen.append(a)
        if cyc:
            best = min(seen, key=lambda b: keys[b >> 1])
            lay(2 * (best >> 1) + 1, len(seen), best >> 1, 1)
            continue
        end1 = a                      # the end reached: its node is left through a side without a link
        a, back = 2 * v, 0
        while link[a] is not None:
            a = link[a] ^ 1
            back += 1
        end0 = a
        L = len(seen) + back
        # a traversal starts at an end and leaves it through the side opposite its dead side
        c0, c1 = _oriented(keys, k, end0 >> 1, end0 & 1), _oriented(keys, k, end1 >> 1, end1 & 1)
        e = end0 if c0 <= c1 else end1
        lay(e ^ 1, L, e >> 1, 0)
    start = sorted(length)
    uid = {s: i for i, s in enumerate(start)}
    seqs = []
    by = {}
    for v in range(n):
        by.setdefault(unitig_start[v], {})[pos[v]] = v
    for s in start:
        nodes = by[s]
        first = dec(_oriented(keys, k, nodes[0], ori[nodes[0]]), k)
        seqs.append(first + "".join(dec(_oriented(keys, k, nodes[p], ori[nodes[p]]), k)[-1] for p in range(1, length[s])))
    return Unitigs([uid[s] for s in unitig_start], pos, ori, start, [length[s] for s in start], [circ[s] for s in start], seqs)


# ---- road B: a walker over strings -------------------------------------------------------------------------------------------------
def unitigs_walk(keys, k):
    strs = [dec(x, k) for x in keys]
    index = {s: i for i, s in enumerate(strs)}

    def node(y):
        i = index.get(y)
        return i if i is not None else index.get(rc_str(y))

    def step(o):      # the oriented k-mer behind o in its unitig, or None
        outs = [o[1:] + c for c in "ACGT" if node(o[1:] + c) is not None]
        if len(outs) != 1:
            return None
        y = outs[0]
        if node(y) == node(o) or o == rc_str(o) or y == rc_str(y):
            return None
        ins = [c + y[:-1] for c in "ACGT" if node(c + y[:-1]) is not None]
        return y if len(ins) == 1 else None

    done = [False] * len(keys)
    found = []      # (start node, oriented k-mers, circular)
    for v, s in enumerate(strs):
        if done[v]:
            continue
        fwd, cyc = [s], False
        while True:
            y = step(fwd[-1])
            if y is None:
                break
            if y == s:
                cyc = True
                break
            fwd.append(y)
        if cyc:
            j = min(range(len(fwd)), key=lambda i: min(fwd[i], rc_str(fwd[i]), key=enc))
            walk = fwd[j:] + fwd[:j]
            if node(walk[0]) is not None and index.get(walk[0]) is None:      # the smallest key was met reversed: go round the other way
                walk = [rc_str(walk[0])] + [rc_str(o) for o in reversed(walk[1:])]
        else:
            bwd = [rc_str(s)]
            while True:
                y = step(bwd[-1])
                if y is None:
                    break
                bwd.append(y)
            walk = [rc_str(o) for o in reversed(bwd[1:])] + fwd
            other = [rc_str(o) for o in reversed(walk)]
            if enc(other[0]) < enc(walk[0]):
                walk = other
        for o in walk:
            done[node(o)] = True
        found.append((node(walk[0]), walk, 1 if cyc else 0))
    found.sort(key=lambda f: f[0])
    n = len(keys)
    unitig, pos, ori = [None] * n, [None] * n, [None] * n
    for u, (_, walk, _) in enumerate(found):
        for p, o in enumerate(walk):
            w = node(o)
            unitig[w], pos[w], ori[w] = u, p, 0 if o == strs[w] else 1
    seqs = [f[1][0] + "".join(o[-1] for o in f[1][1:]) for f in found]
    return Unitigs(unitig, pos, ori, [f[0] for f in found], [len(f[1]) for f in found], [f[2] for f in found], seqs)


# ---- the worked examples of the header ---------------------------------------------------------------------------------------------
EX_LINEAR = dict(k=5, keys=(173, 267, 316, 365, 436, 692, 721), strs=("ATTGC", "CAATG", "CAGGA", "CCTGC", "CTGCA", "TTGCA", "TGCAC"), U=3,
                 seqs=["CATTGCA", "TCCTGCA", "TGCAC"], unitig=[0, 0, 1, 1, 1, 0, 2], pos=[1, 0, 0, 1, 2, 2, 0], ori=[0, 1, 1, 0, 0, 0, 0],
                 start=[1, 2, 6], len=[3, 3, 1], circ=[0, 0, 0])
EX_CIRCULAR = dict(k=5, strs=("ACCTG", "AGGTC", "CCTGA", "CTGAC", "TGACC"), U=1, seqs=["ACCTGACCT"], pos=[0, 4, 1, 2, 3], ori=[0, 1, 0, 0, 0],
                   circ=[1])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def kmers_of(seq, k, circular=False):
    """the distinct canonical k-mers of seq (of the circle seq closes, when circular), ascending"""
    if circular:
        seq = (seq * (k // len(seq) + 2))[:len(seq) + k - 1]
    return sorted({canon_int(enc(seq[i:i + k]), k) for i in range(len(seq) - k + 1)})


def ordered(keys, rng, shuffle):
    keys = list(keys)
    if shuffle:
        rng.shuffle(keys)
    return keys


K_SWEEP = (8, 12, 31, 32, 33, 63, 64, 65, 96, 97, 126, 127)
PATH_L = (1, 2, 3, 4, 5, 8, 9, 16, 17, 1023, 1024, 1025, 4097)
CYCLE_L = (2, 3, 4, 5, 64, 65, 1024, 1025)
PAL_K = (8, 32, 64, 96, 126)      # an even k of every key_words class (1, 1, 2, 3, 4)

_cases = None


def single_path(n, k=31):
    """n k-mers of a random string that make one path (the seed is searched for, the CPU test asserts U == 1)"""
    for seed in range(64):
        rng = random.Random(1000 * n + seed)
        keys = kmers_of(rand_seq(rng, n + k - 1), k)
        if len(keys) == n and unitigs_links(keys, k).U == 1:
            return ordered(keys, rng, True)
    raise AssertionError(f"no single path of {n}")


def single_cycle(n, k=31):
    for seed in range(256):
        rng = random.Random(7000 * n + seed)
        keys = kmers_of(rand_seq(rng, n), k, circular=True)
        if len(keys) != n:
            continue
        r = unitigs_links(keys, k)
        if r.U == 1 and r.circ == [1]:
            return ordered(keys, rng, True)
    raise AssertionError(f"no single cycle of {n}")


def cases():
    """[(name, k, keys)]: keys a list of distinct canonical integers in the order the call gets them"""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    # the sweep of k: a random sequence with a repeat and an inverted repeat planted, shuffled and sorted in turn
    for i, k in enumerate(K_SWEEP):
        rng = random.Random(100 + k)
        a, rep = rand_seq(rng, 150), rand_seq(rng, k + 6)
        seq = a[:50] + rep + a[50:100] + rep + a[100:] + rc_str(rep) + rand_seq(rng, 40)
        out.append((f"seq_k{k}_{'shuffled' if i % 2 == 0 else 'sorted'}", k, ordered(kmers_of(seq, k), rng, i % 2 == 0)))
    # a palindromic node with neighbours
    for k in PAL_K:
        rng = random.Random(200 + k)
        h = rand_seq(rng, k // 2)
        out.append((f"palindrome_k{k}", k, ordered(kmers_of(rand_seq(rng, 30) + h + rc_str(h) + rand_seq(rng, 30), k), rng, True)))
    # a homopolymer (a self-loop) and a hairpin (w + rc(w): at odd k the k-mer astride the centre is followed by its own reverse complement)
    rng = random.Random(300)
    out.append(("homopolymer_k12", 12, ordered(kmers_of(rand_seq(rng, 25) + "A" * 16 + rand_seq(rng, 25), 12), rng, True)))
    w = rand_seq(rng, 30)
    out.append(("hairpin_k11", 11, ordered(kmers_of(rand_seq(rng, 20) + w + rc_str(w) + rand_seq(rng, 20), 11), rng, True)))
    out.append(("hairpin_k33", 33, ordered(kmers_of(rand_seq(rng, 20) + w + rc_str(w) + rand_seq(rng, 20), 33), rng, True)))
    # dense random keys: sides of every degree
    rng = random.Random(400)
    out.append(("dense_k8", 8, ordered({canon_int(rng.getrandbits(16), 8) for _ in range(9000)}, rng, True)))
    # several circles and paths in one call
    rng = random.Random(500)
    mix = set()
    for n in (7, 40, 3, 90):
        mix |= set(kmers_of(rand_seq(rng, n), 31, circular=True))
    mix |= set(kmers_of(rand_seq(rng, 300), 31))
    out.append(("mixed_k31", 31, ordered(mix, rng, True)))
    for n in PATH_L:
        out.append((f"path_{n}", 31, single_path(n)))
    for n in CYCLE_L:
        out.append((f"cycle_{n}", 31, single_cycle(n)))
    for k in (64, 97):      # circles at wider keys
        rng = random.Random(600 + k)
        out.append((f"cycle_k{k}", k, ordered(kmers_of(rand_seq(rng, 50), k, circular=True), rng, True)))
    _cases = out
    return out


_results = {}


def expected(name):
    """road A's result for the case, computed once and shared"""
    if name not in _results:
        for nm, k, keys in cases():
            if nm == name:
                _results[name] = unitigs_links(keys, k)
    return _results[name]


# ---- kmx_groupsum_* ------------------------------------------------------------------------------------------------------------------
MODE_COUNT, MODE_PA = 0, 1


def make_body(rng, n_rows, n_cols, key_words, mode, density=0.4, big=False):
    """a matrix body: (bytes, counts uint32[n_rows, n_cols]); PA bodies get their padding bits SET, so that a kernel that lets them through shows"""
    counts = (rng.random((n_rows, n_cols)) < density) * rng.integers(1, 1000, (n_rows, n_cols))
    counts = counts.astype(np.uint32)
    if big:
        counts[counts > 0] = 0xFFFFFFFF
    if mode == MODE_PA:
        counts = (counts > 0).astype(np.uint32)
    keys = rng.integers(0, 2 ** 63, (n_rows, key_words), dtype=np.uint64)
    rows = []
    for r in range(n_rows):
        if mode == MODE_COUNT:
            rows.append(keys[r].tobytes() + counts[r].tobytes())
        else:
            nb = (n_cols + 7) // 8
            bits = np.ones(nb * 8, np.uint8)
            bits[:n_cols] = counts[r]
            rows.append(keys[r].tobytes() + np.packbits(bits, bitorder="little").tobytes())
    return b"".join(rows), counts


def groupsum_np(counts, groups, cols, min_abund, g0, n_groups, mode, want_sums):
    """-> (size uint32[G], present uint32[G, M], sums uint64[G, M] or None)"""
    cols = np.arange(counts.shape[1]) if cols is None else np.asarray(cols)
    M = len(cols)
    size, present = np.zeros(n_groups, np.uint32), np.zeros((n_groups, M), np.uint32)
    sums = np.zeros((n_groups, M), np.uint64) if want_sums else None
    groups = np.asarray(groups, np.int64)
    inw = (groups >= g0) & (groups < g0 + n_groups)
    g = groups[inw] - g0
    sub = counts[inw][:, cols]
    pres = sub >= min_abund if mode == MODE_COUNT else sub > 0
    np.add.at(size, g, 1)
    np.add.at(present, g, pres.astype(np.uint32))
    if want_sums:
        np.add.at(sums, g, np.where(pres, sub, 0).astype(np.uint64))
    return size, present, sums


def groupsum_loops(counts, groups, cols, min_abund, g0, n_groups, mode, want_sums):
    cols = list(range(counts.shape[1])) if cols is None else list(cols)
    M = len(cols)
    size, present = [0] * n_groups, [[0] * M for _ in range(n_groups)]
    sums = [[0] * M for _ in range(n_groups)] if want_sums else None
    for r, g in enumerate(groups):
        g = int(g)
        if not g0 <= g < g0 + n_groups:
            continue
        size[g - g0] += 1
        for j, c in enumerate(cols):
            v = int(counts[r][c])
            if (v >= min_abund) if mode == MODE_COUNT else v > 0:
                present[g - g0][j] += 1
                if want_sums:
                    sums[g - g0][j] += v
    return (np.array(size, np.uint32), np.array(present, np.uint32).reshape(n_groups, M),
            np.array(sums, np.uint64).reshape(n_groups, M) if want_sums else None)


# ---- the driver's file formats ----------------------------------------------------------------------------------------------------
def parse_kmers(text, k):
    """the first tab-separated field of every line that is not empty, does not start with # and is not the header `kmer ...`, canonical -> a set of integers; ValueError
    for a field that is no k-mer of the run's k"""
    out = set()
    for ln, line in enumerate(text.split("\n"), 1):
        line = line.rstrip("\r")
        if not line or line[0] == "#":
            continue
        s = line.split("\t")[0]
        if s == "kmer":      # the header line of kmx diff / kmx assoc
            continue
        if len(s) != k:
            raise ValueError(f"line {ln}: a k-mer of {len(s)} characters")
        if any(c not in "ACGTacgt" for c in s):
            raise ValueError(f"line {ln}: malformed k-mer")
        out.add(canon_int(enc(s.upper()), k))
    return out


def fasta_text(r, k):
    return "".join(f">{u} LN:i:{r.len[u] + k - 1} KM:i:{r.len[u]}{' CL:Z:circular' if r.circ[u] else ''}\n{r.seqs[u]}\n" for u in range(r.U))


def table_text(ids, size, present, sums, value):
    """size [U], present / sums [U, M] as groupsum gives them over the whole id range"""
    lines = ["unitig\tkmers\t" + "\t".join(ids) + "\n"]
    for u in range(len(size)):
        if value == "sum":
            vals = [str(int(v)) for v in sums[u]]
        elif value == "present":
            vals = [str(int(v)) for v in present[u]]
        elif value == "mean":
            vals = ["%.2f" % (float(int(v)) / float(int(size[u]))) for v in sums[u]]
        else:
            vals = ["%.2f" % (float(int(v)) / float(int(size[u]))) for v in present[u]]
        lines.append(f"{u}\t{int(size[u])}\t" + "\t".join(vals) + "\n")
    return "".join(lines)


def driver_expected(bodies, n_cols, key_words, mode, k, kmers=None, cols=None, min_abund=1, value=None, ids=None):
    """what `kmx unitigs` writes for a run's bodies -> (FASTA text, table text, listed k-mers the run lacks)"""
    rb = 8 * key_words + (4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8)
    keys, pay = [], []
    for b in bodies:
        a = np.frombuffer(bytes(b), np.uint8).reshape(-1, rb)
        for row in a:
            key = int.from_bytes(row[:8 * key_words].tobytes(), "little")
            if kmers is not None and key not in kmers:
                continue
            keys.append(key)
            p = row[8 * key_words:]
            pay.append(np.frombuffer(p.tobytes(), "<u4") if mode == MODE_COUNT else np.unpackbits(p, bitorder="little")[:n_cols].astype(np.uint32))
    r = unitigs_links(keys, k)
    counts = np.array(pay, np.uint32).reshape(len(keys), n_cols)
    value = value or ("mean" if mode == MODE_COUNT else "frac")
    size, present, sums = groupsum_np(counts, r.unitig, cols, min_abund, 0, max(r.U, 1), mode, mode == MODE_COUNT)
    ids = ids if cols is None else [ids[c] for c in cols]
    table = table_text(ids, size[:r.U], present[:r.U], None if sums is None else sums[:r.U], value)
    return fasta_text(r, k), table, 0 if kmers is None else len(kmers - set(keys))
