"""Reads whose k-mers tie in their leading words: the count sort's compares, shuffles, radix passes and run boundaries decided by the
LOWER words of a key (amplicon reads, reads behind a primer, tandem repeats: thousands of distinct k-mers that share their first
bases).  Shared by test_count_tied_cpu.py and test_count_tied_gpu.py.

A batch is reads of exactly k bases, `S + tail`: S a fixed prefix of `tie` bases that begins AAC (the forward strand is the canonical one:
the tails do not end in T, so the reverse complement does not begin with A), the tails distinct and random; a fixed share of them is given
two and three times (hard-min 2 keeps a proper subset); a few hundred random 150-base reads beside them (a partition has tens of buckets).
The minimizers inside the tails spread a batch over the partitions, so the size of the tied group is MEASURED, from the oracle's output
(`describe`), and the (k, tie, n, seed) of CASES were searched until it lay in the class the case names."""
import numpy as np

import orc

M, P = 10, 4
BACKGROUND = 400                   # random 150-base reads beside the tied ones
DUP = (0.2, 0.1)                   # share of the tails given twice / three times

# count_sort.hpp's constants, restated (the classes the bucket kernels distinguish: cs_launch_bucket_count*)
CS_TARGET = 416                    # aimed bucket size: a partition of more keys has several buckets
WAVE_SMALL, WAVE_MAX = 512, 1024   # k_cs_wave_sort<K, 8, 16>: the small and the large register network
LDS_MID = 2048                     # k_cs_sort<K, 2048> (128-bit keys: the first of two launches; wide keys: the last)
CAP = {"u64": 4096, "u128": 4096, "wide3": 2048, "wide4": 2048}      # CsCap<K>::cap -- beyond: the overflow word, the library passes
CS_LUT = 1024                      # cells of the bucket look-up table (64-bit keys, the sync-free path)
KEY_TYPES = ("u64", "u128", "wide3", "wide4")


def key_type(k):
    return "u64" if k <= 32 else "u128" if k <= 64 else "wide3" if k <= 96 else "wide4"


def classes_of(kt):
    return ["<=512", "513-1024", "1025-2048"] + (["2049-4096"] if CAP[kt] == 4096 else []) + ["above-cap"]


def size_class(kt, g):
    if g > CAP[kt]:
        return "above-cap"
    return "<=512" if g <= WAVE_SMALL else "513-1024" if g <= WAVE_MAX else "1025-2048" if g <= LDS_MID else "2049-4096"


def tshift_of(k):
    """count.hip, fast_tail_impl: the table looks at 32 bits of a 64-bit key from here on (its top 16 bases)"""
    return max(0, 2 * k - 32)


_PREFIX = "AAC" + "".join(np.random.default_rng(20240).choice(list("ACGT"), size=125))


def background(seed, n=BACKGROUND, length=150):
    rng = np.random.default_rng(seed)
    return ["".join(r) for r in rng.choice(list("ACGT"), size=(n, length))]


def tied_batch(k, tie, n, seed, dup=DUP, n_background=BACKGROUND):
    """-> reads: n distinct `S + tail` of k bases (the first dup[0] * n of them twice, the next dup[1] * n three times), shuffled, and the
    background reads behind them"""
    assert 1 <= tie < k <= 127
    rng = np.random.default_rng(seed)
    S, tl = _PREFIX[:tie], k - tie
    tails, seen = [], set()
    while len(tails) < n:
        for row in rng.integers(0, 4, size=(2 * n, tl)):
            if row[-1] == 2:           # (A0 C1 T2 G3: no tail ends in T)
                continue
            t = "".join("ACTG"[x] for x in row)
            if t not in seen:
                seen.add(t); tails.append(t)
                if len(tails) == n:
                    break
        assert 3 * 4 ** (tl - 1) >= n, "not that many tails"
    n2, n3 = int(dup[0] * n), int(dup[1] * n)
    reads = [S + t for t in tails] + [S + t for t in tails[:n2 + n3]] + [S + t for t in tails[n2:n2 + n3]]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    return reads + background(seed + 1, n_background)


def exclusive_table(tied, rest, k, part=P - 1):
    """a repartition table that gives partition `part` the tied reads' k-mers alone: the static table over the partitions below it, the tied
    reads' minimizers sent to `part` (as test_count_keyspace_gpu.dataset does), and the other reads that hold one of those dropped
    -> (table, the reads kept)"""
    lut, rep = orc.minimizer_lut(M), orc.repart_static(M, part)
    for r in set(tied):
        rep[orc.minimizer_of(orc.kmer_from_string(r), k, M, lut)] = part
    kept = [r for r in rest if orc.superk_partition([r], k, M, lut, rep, P)[part][1] == 0]
    return rep, kept


def splitter_rows(keys, k):
    """what the sample sort's splitters see of sorted keys [n, kw] (low word first): wide keys their two most significant words, 128-bit
    keys here the high word, 64-bit keys the 32 table bits"""
    kt = key_type(k)
    if kt == "u64":
        return ((keys[:, :1] >> np.uint64(tshift_of(k))) & np.uint64(0xFFFFFFFF))
    if kt == "u128":
        return keys[:, 1:2]
    return keys[:, -2:]


def _largest_run(rows):
    """rows [n, w] with equal rows adjacent -> (start, length) of the longest run of equal rows"""
    n = len(rows)
    if n == 0:
        return 0, 0
    cut = np.concatenate([[0], 1 + np.nonzero((rows[1:] != rows[:-1]).any(axis=1))[0], [n]])
    i = int(np.argmax(np.diff(cut)))
    return int(cut[i]), int(cut[i + 1] - cut[i])


def describe(streams, k):
    """the batch as the oracle sees it.  Per partition stream: nkeys (k-mers, repeats counted), distinct; the largest group of distinct
    keys that agree in the splitter (`group`) and the k-mers it stands for, repeats counted (`group_keys`: what a bucket holds, and what
    the size classes are about), the words in which neighbours of the sorted group first differ (`words`, a set), the share of the group
    that hard-min 2 keeps (`kept2`); wide keys: the largest group that agrees in the top word alone (`top_group`); 64-bit
    keys: the distinct table values of the partition (`tvals`) and their span (`tspan` = largest - smallest)"""
    out = []
    for recs, nk, _ in streams:
        keys, counts = orc.count_kmer(recs, k, 1)
        kw = keys.shape[1] if keys.ndim == 2 else 1
        keys = keys.reshape(len(counts), kw)
        d = dict(nkeys=int(nk), distinct=len(counts), group=0, group_keys=0, words=set(), kept2=0.0)
        if len(counts):
            s, g = _largest_run(splitter_rows(keys, k))
            grp = keys[s:s + g]
            differ = grp[1:] != grp[:-1]                                    # [g - 1, kw]
            d["group"], d["group_keys"], d["kept2"] = g, int(counts[s:s + g].sum()), float((counts[s:s + g] >= 2).mean())
            d["words"] = set((kw - 1 - np.argmax(differ[:, ::-1], axis=1)).tolist())
            if kw >= 3:
                s, g = _largest_run(keys[:, -1:])
                differ = keys[s + 1:s + g] != keys[s:s + g - 1]
                d["top_group"], d["top_words"] = g, set((kw - 1 - np.argmax(differ[:, ::-1], axis=1)).tolist())
            if kw == 1:
                t = splitter_rows(keys, k)[:, 0]
                d["tvals"], d["tspan"] = len(np.unique(t)), int(t.max() - t.min())
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the sweep
# kind: "tied"      the group agrees in the splitter and first differs in word `word` (64-bit keys: below the table bits; k = 16: the
#                   table bits are the key, a group is one key)
#       "top-only"  wide keys that agree in the top word alone: the splitters' second word decides, the group spreads over buckets
#       "lut-..."   k <= 32, partition P - 1 holds tied k-mers only (exclusive_table): every key shares its table bits ("lut-same": tmin ==
#                   tmax), their span is below CS_LUT ("lut-narrow": lsh == 0) or 1024 ... 4095 ("lut-wide": lsh 1 or 2)
# cls: the size class of the largest tied group's k-mers, repeats counted (classes_of);  (k, tie, n, seed) found by search: see DESIGN.md
def _c(kind, k, tie, n, seed, cls, word=0):
    return dict(kind=kind, k=k, tie=tie, n=n, seed=seed, cls=cls, word=word, id=f"{kind}-k{k}-tie{tie}-n{n}")


CASES = [
    # WideKey<3>: the group first differs in word 0
    _c("tied", 96, 64, 2600, 1, "above-cap"),
    _c("tied", 96, 64, 250, 1, "<=512"),
    _c("tied", 80, 48, 610, 1, "513-1024"),
    _c("tied", 65, 33, 1240, 1, "1025-2048"),
    _c("top-only", 96, 40, 4000, 1, "<=512", word=1),
    # WideKey<4>: word 1, and word 0 only
    _c("tied", 127, 63, 3600, 1, "above-cap", word=1),
    _c("tied", 127, 95, 2600, 1, "above-cap"),
    _c("tied", 127, 120, 525, 1, "513-1024"),
    _c("tied", 111, 47, 1510, 1, "1025-2048", word=1),
    _c("tied", 97, 70, 250, 1, "<=512"),
    _c("top-only", 127, 40, 4000, 1, "<=512", word=2),
    # __uint128_t: the high word ties, the low word decides (k = 33: the high word is the first base -- every k-mer that begins with A ties)
    _c("tied", 33, 20, 4000, 1, "above-cap"),
    _c("tied", 63, 31, 2470, 1, "2049-4096"),
    _c("tied", 47, 15, 1200, 1, "1025-2048"),
    _c("tied", 47, 30, 550, 1, "513-1024"),
    _c("tied", 63, 40, 220, 1, "<=512"),
    # u64: the 32 table bits (the top 16 bases) tie
    _c("tied", 31, 16, 3400, 1, "above-cap"),
    _c("tied", 32, 16, 2170, 1, "2049-4096"),
    _c("tied", 32, 20, 1080, 1, "1025-2048"),
    _c("tied", 31, 25, 525, 1, "513-1024"),
    _c("tied", 31, 20, 220, 1, "<=512"),
    _c("tied", 16, 8, 332, 1, "<=512"),
    # the bucket look-up table's corners: partition P - 1 holds the tied k-mers alone
    _c("lut-same", 31, 16, 2750, 1, "2049-4096"),
    _c("lut-narrow", 31, 11, 3575, 1, "<=512"),
    _c("lut-wide", 32, 10, 3575, 1, "<=512"),
]


_BATCH = {}


def batch(case):
    """-> (reads, repartition table, oracle streams [(records, k-mers, super-k-mers)] per partition, describe()); computed once a case"""
    key = case["id"]
    if key not in _BATCH:
        k = case["k"]
        lut = orc.minimizer_lut(M)
        if case["kind"].startswith("lut-"):
            reads = tied_batch(k, case["tie"], case["n"], case["seed"], n_background=0)
            rep, rest = exclusive_table(reads, background(case["seed"] + 1), k)
            reads = reads + rest
        else:
            reads, rep = tied_batch(k, case["tie"], case["n"], case["seed"]), orc.repart_static(M, P)
        streams = orc.superk_partition(reads, k, M, lut, rep, P)
        _BATCH[key] = (reads, rep, streams, describe(streams, k))
    return _BATCH[key]


def tied_partition(case):
    """the partition whose tied group is the case's: the exclusive one of a look-up table case, else the one with the largest group"""
    if case["kind"].startswith("lut-"):
        return P - 1
    desc = batch(case)[3]
    return max(range(P), key=lambda p: desc[p]["top_group" if case["kind"] == "top-only" else "group"])
